"""Recurrent language model for decoding (mirror of RNNLM / ClassifierWithState, model/lm.py:26-146), decode side only.

Shallow fusion in the beam search (Decoder.recognize_beam(..., rnnlm=...)) asks the LM for the log-probabilities of the next
label after every live hypothesis.  Unlike upstream -- one hypothesis per ``predict`` call -- all ``n`` live hypotheses of a
position go through ONE call: ``x`` holds their last labels, the state tensors are (n, n_units) and stay on the GPU.

A position is 1 .. ``beam`` rows against the whole model (two 650-unit LSTM cells and a 4233 x 650 output layer in the recipe:
34 MB of fp32 weights), so the step runs on the few-row kernels of csrc/rnnlm.hip -- re2e_lm_lstm_cell (embedding gather +
both gate products + the cell in one launch, once per layer), re2e_lm_output, re2e_lm_log_softmax_combine -- which stream the
weights through registers once.  ``COMPOSED_PATH`` swaps in the same arithmetic over the library's general entry points
(re2e_embedding_fwd, re2e_gemm x 5, re2e_lstm_cell_fwd x 2, re2e_log_softmax_rows): the tests' arbiter and the timing baseline
(tools/bench_recog_lm.py), not a user option.

Word-level LMs (LookAheadWordLM, MultiLevelLM: model/extlm.py here) are predictors over one or two RNNLMs; they return log-probabilities
(``normalized``) and take the labels the search holds on the host (``host_labels``, the ``labels=`` of ``predict_combined``).

Out of scope: training the LM (lm_train.py, lm.train, the loss of ClassifierWithState.forward), the FS-RNN LM, n-gram / FST LMs
(NgramCharacterKenLM), deep and cold fusion."""
import numpy as np
import torch

from .. import ops
from ..lib import Re2eError, call, ptr
from .e2e_common import LinearParams, host_to_dev
from .e2e_decoder import EmbeddingParams, LSTMCellParams

COMPOSED_PATH = False          # tests / tools: the step over the general entry points instead of csrc/rnnlm.hip (arbiter, timing baseline)
FUSED_MAX_ROWS = 64            # re2e_lm_*: 1 <= n <= 64; more rows take the composed path

STATE_KEYS = ('c1', 'h1', 'c2', 'h2')


def _empty(*shape, **kw):
    """Every output buffer of a step comes from here (tests hand out NaN-filled ones: a kernel must write all of it)."""
    return torch.empty(*shape, **kw)


class RNNLM(torch.nn.Module):
    """Parameter holder with the reference's state_dict names: embed.weight (V, I), l1 / l2 .weight_ih / .weight_hh / .bias_ih /
    .bias_hh (nn.LSTMCell), lo.weight (V, H), lo.bias; all initialised uniform(-0.1, 0.1) (lm.py:125-133).  Evaluation only:
    dropout is the identity there and ``forward`` in training mode raises (training the LM is out of scope)."""

    def __init__(self, n_vocab, input_units, n_units, dropout_rate=0.5, embed_vecs_init=None):
        super(RNNLM, self).__init__()
        self.n_vocab, self.input_units, self.n_units, self.dropout_rate = n_vocab, input_units, n_units, dropout_rate
        self.embed = EmbeddingParams(n_vocab, input_units)
        self.l1 = LSTMCellParams(input_units, n_units)
        self.l2 = LSTMCellParams(n_units, n_units)
        self.lo = LinearParams(n_units, n_vocab)
        for param in self.parameters():
            param.data.uniform_(-0.1, 0.1)
        if embed_vecs_init is not None:
            self.embed.weight.data.copy_(torch.from_numpy(np.asarray(embed_vecs_init)))

    def zero_state(self, batchsize):
        return torch.zeros(batchsize, self.n_units, device=self.lo.weight.device)

    def _ids(self, x):
        dev = self.lo.weight.device
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.to(device=dev, dtype=torch.int32).contiguous().view(-1)
        return host_to_dev(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, np.int32).reshape(-1), dev)

    def _state(self, state, n):
        if state is None:
            return None
        st = tuple(state[k] for k in STATE_KEYS)
        for t in st:
            if tuple(t.shape) != (n, self.n_units):
                raise Re2eError('RNNLM state is %s, expected (%d, %d): one row per label in x' % (tuple(t.shape), n, self.n_units))
        return tuple(t.contiguous() for t in st)

    def forward(self, state, x):
        """``x``: the n last labels; ``state``: {'c1', 'h1', 'c2', 'h2'} of (n, n_units) each or None (zeros) -> (state, logits (n, V))."""
        if self.training:
            raise Re2eError('RNNLM runs in evaluation mode only (call .eval()): training the LM is out of scope')
        if not self.lo.weight.is_cuda:
            raise Re2eError('RNNLM parameters are on %s: there is no CPU path (call .cuda())' % self.lo.weight.device)
        ids = self._ids(x)
        n = ids.numel()
        if n < 1:
            raise Re2eError('RNNLM.forward needs at least one label')
        with torch.no_grad():
            st = self._state(state, n)
            if COMPOSED_PATH or n > FUSED_MAX_ROWS:
                return self._forward_composed(st, ids, n)
            return self._forward_fused(st, ids, n)

    def _forward_fused(self, st, ids, n):
        dev, V, I, H = ids.device, self.n_vocab, self.input_units, self.n_units
        c1, h1, c2, h2 = st if st is not None else (None,) * 4
        new = _empty(4, n, H, device=dev)                       # c1, h1, c2, h2
        l1, l2 = self.l1, self.l2
        call('re2e_lm_lstm_cell', ptr(self.embed.weight), I, ids.data_ptr(), V, I, ptr(l1.weight_ih), ptr(l1.weight_hh), ptr(l1.bias_ih),
             ptr(l1.bias_hh), ptr(h1), ptr(c1), n, H, new[1].data_ptr(), new[0].data_ptr())
        call('re2e_lm_lstm_cell', new[1].data_ptr(), H, None, 0, H, ptr(l2.weight_ih), ptr(l2.weight_hh), ptr(l2.bias_ih), ptr(l2.bias_hh),
             ptr(h2), ptr(c2), n, H, new[3].data_ptr(), new[2].data_ptr())
        logits = _empty(n, V, device=dev)
        call('re2e_lm_output', new[3].data_ptr(), ptr(self.lo.weight), ptr(self.lo.bias), n, V, H, logits.data_ptr())
        return dict(zip(STATE_KEYS, new.unbind(0))), logits

    def _forward_composed(self, st, ids, n):
        dev, V, I, H = ids.device, self.n_vocab, self.input_units, self.n_units
        c1, h1, c2, h2 = st if st is not None else (torch.zeros(n, H, device=dev),) * 4
        emb = _empty(n, I, device=dev)
        call('re2e_embedding_fwd', ptr(self.embed.weight), ids.data_ptr(), n, I, emb.data_ptr(), I)
        new = _empty(4, n, H, device=dev)
        for x, lay, h, c, k in ((emb, self.l1, h1, c1, 0), (new[1], self.l2, h2, c2, 2)):
            gates = _empty(n, 4 * H, device=dev)
            ops.gemm(x, lay.weight_ih, gates, n, 4 * H, x.shape[1], transb=True, bias=lay.bias_ih, bias2=lay.bias_hh)
            ops.gemm(h, lay.weight_hh, gates, n, 4 * H, H, transb=True, beta=1.0)
            call('re2e_lstm_cell_fwd', gates.data_ptr(), c.data_ptr(), new[k].data_ptr(), new[k + 1].data_ptr(), n, H)
        logits = _empty(n, V, device=dev)
        ops.gemm(new[3], self.lo.weight, logits, n, V, H, transb=True, bias=self.lo.bias)
        return dict(zip(STATE_KEYS, new.unbind(0))), logits


class ClassifierWithState(torch.nn.Module):
    """lm.py:26-109, decode side: ``predict(state, x) -> (state, log_probs (n, V))``.  Its parameters are ``predictor.*``, so a
    checkpoint the reference wrote loads with a strict ``load_state_dict``.  The training loss (``forward``) is out of scope."""

    def __init__(self, predictor, lossfun=None, accfun=None, label_key=-1):
        if not isinstance(label_key, (int, str)):
            raise TypeError('label_key must be int or str, but is %s' % type(label_key))
        super(ClassifierWithState, self).__init__()
        self.lossfun, self.accfun, self.label_key = lossfun, accfun, label_key
        self.y, self.loss, self.accuracy = None, None, None
        self.predictor = predictor

    def forward(self, state, *args, **kwargs):
        raise Re2eError('ClassifierWithState.forward is the LM training loss (lm_train.py): out of scope, use predict()')

    def predict(self, state, x, labels=None):
        state, lp, _ = self.predict_combined(state, x, labels=labels)
        return state, lp

    def predict_combined(self, state, x, att=None, lm_weight=0.0, labels=None):
        """``predict`` plus, when ``att`` (n, V) is given, ``att + lm_weight * log_probs`` (the shallow-fusion score of
        e2e_decoder.py:272, product and sum each rounded to fp32) from the same pass over the rows: (state, log_probs, combined).
        ``labels``: the labels of ``x`` as a host array, for the predictors that branch on them (``host_labels``: model/extlm.py)."""
        if labels is not None and getattr(self.predictor, 'host_labels', False):
            state, z = self.predictor(state, x, labels=labels)
        else:
            state, z = self.predictor(state, x)
        if getattr(self.predictor, 'normalized', False):
            return state, z, (att + float(np.float32(lm_weight)) * z if att is not None else None)
        n, V = z.shape
        lp = _empty(n, V, device=z.device)
        if COMPOSED_PATH or not isinstance(self.predictor, RNNLM):
            call('re2e_log_softmax_rows', z.data_ptr(), n, V, V, lp.data_ptr())
            return state, lp, (att + float(np.float32(lm_weight)) * lp if att is not None else None)
        comb = _empty(n, V, device=z.device) if att is not None else None
        call('re2e_lm_log_softmax_combine', z.data_ptr(), n, V, ptr(att), float(np.float32(lm_weight)), lp.data_ptr(), ptr(comb))
        return state, lp, comb
