"""Recurrent language model (mirror of RNNLM / ClassifierWithState / train, model/lm.py:26-340): decoding and training.

Decoding.  Shallow fusion in the beam search (Decoder.recognize_beam(..., rnnlm=...)) asks the LM for the log-probabilities of the next
label after every live hypothesis.  Unlike upstream -- one hypothesis per ``predict`` call -- all ``n`` live hypotheses of a
position go through ONE call: ``x`` holds their last labels, the state tensors are (n, n_units) and stay on the GPU.

A position is 1 .. ``beam`` rows against the whole model (two 650-unit LSTM cells and a 4233 x 650 output layer in the recipe:
34 MB of fp32 weights), so the step runs on the few-row kernels of csrc/rnnlm.hip -- re2e_lm_lstm_cell (embedding gather +
both gate products + the cell in one launch, once per layer), re2e_lm_output, re2e_lm_log_softmax_combine -- which stream the
weights through registers once.  ``COMPOSED_PATH`` swaps in the same arithmetic over the library's general entry points
(re2e_embedding_fwd, re2e_gemm x 5, re2e_lstm_cell_fwd x 2, re2e_log_softmax_rows): the tests' arbiter and the timing baseline
(tools/bench_recog_lm.py), not a user option.

Word-level LMs (LookAheadWordLM, MultiLevelLM: model/extlm.py here) are predictors over one or two RNNLMs; they return log-probabilities
(``normalized``) and take the labels the search holds on the host (``host_labels``, the ``labels=`` of ``predict_combined``).  N-gram
back-off LMs (the reference's NgramCharacterKenLM / --kenlm) are model/ngram.py: ``NgramLM`` is a predictor over flat ARPA tables, one
launch per position, which also returns the shallow-fusion sum (``forward_combined``).

Training (lm_train.py, ``train`` / ``evaluate`` below).  A truncated-BPTT window of T steps x B rows runs as ONE pass,
``RNNLM.forward_seq``: embedding -> dropout -> the W_ih product of all T*B rows (both biases in its epilogue) -> the recurrence
(ops.lm_lstm_seq: csrc/lmseq.hip, one fused product + cell launch per step, state carried in and out with its gradient) -> dropout ->
layer 2 -> dropout -> output layer; the three dropouts are three counter-based masks over the whole (T, B, .) tensors (ops.dropout), not
torch's RNG stream.  ``RNNLM.forward`` in training mode is that window with T = 1, so the reference's per-step loop (sum 35 losses,
backward, detach) works and chains through the state's gradient; ``ClassifierWithState.forward_seq`` is the trainer's path.  The output
layer, the cross-entropy and their backward run over row blocks when T*B*V would pass ``OUTPUT_MAX_ELEMS`` (the kernels address their
operands with 32-bit element offsets).  In training ``COMPOSED_PATH`` means the same window with re2e_gemm + re2e_lstm_cell_fwd / _bwd
per step as its recurrence (tools/bench_lm_train.py).

Out of scope (refused with Re2eError where they can be asked for): the FS-RNN LM in ``train`` (--lm-type fsrnnlm is trained by
model/fsrnn.py, not by this function; ``ClassifierWithState`` and ``evaluate`` take an FSRNNLM predictor as they take an RNNLM), training on
several GPUs or on the CPU, FST LMs (model/fstlm.py upstream) and n-gram LMs in KenLM's binary format (ARPA files: model/ngram.py), deep and
cold fusion."""
import logging
import os

import numpy as np
import torch

from .. import ops
from ..lib import Re2eError, call, ptr
from .e2e_common import LinearParams, host_to_dev
from .e2e_decoder import EmbeddingParams, LSTMCellParams

COMPOSED_PATH = False          # tests / tools: the step over the general entry points instead of csrc/rnnlm.hip (arbiter, timing baseline)
FUSED_MAX_ROWS = 64            # re2e_lm_*: 1 <= n <= 64; more rows take the composed path
OUTPUT_MAX_ELEMS = 2 ** 31 - 1  # training: logits per output-layer / cross-entropy call (32-bit element offsets); more rows go in blocks

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
        if not self.lo.weight.is_cuda:
            raise Re2eError('RNNLM parameters are on %s: there is no CPU path (call .cuda())' % self.lo.weight.device)
        ids = self._ids(x)
        if self.training:
            state, logits = self.forward_seq(state, ids.view(1, -1))
            return state, logits[0]
        n = ids.numel()
        if n < 1:
            raise Re2eError('RNNLM.forward needs at least one label')
        with torch.no_grad():
            st = self._state(state, n)
            if COMPOSED_PATH or n > FUSED_MAX_ROWS:
                return self._forward_composed(st, ids, n)
            return self._forward_fused(st, ids, n)

    def window(self, state, xs):
        """One truncated-BPTT window up to the output layer: ``xs`` (T, B) labels -> (state, hidden (T*B, n_units) after the last
        dropout).  ``state`` carries autograd history: detach it between windows (the trainer does)."""
        if not self.lo.weight.is_cuda:
            raise Re2eError('RNNLM parameters are on %s: there is no CPU path (call .cuda())' % self.lo.weight.device)
        if not hasattr(xs, 'shape') or len(xs.shape) != 2 or xs.shape[0] < 1 or xs.shape[1] < 1:
            raise Re2eError('RNNLM.forward_seq takes labels of shape (T, B)')
        T, B = int(xs.shape[0]), int(xs.shape[1])
        ids = self._ids(xs)
        st = self._state(state, B)
        if st is None:
            st = (self.zero_state(B),) * 4
        c1, h1, c2, h2 = st
        p = self.dropout_rate if self.training else 0.0
        H = self.n_units
        x = ops.dropout(ops.embedding(self.embed.weight, ids), p)
        xg = ops.linear_2bias(x, self.l1.weight_ih, self.l1.bias_ih, self.l1.bias_hh)
        y1, h1, c1 = ops.lm_lstm_seq(xg.view(T, B, 4 * H), self.l1.weight_hh, h1, c1, composed=COMPOSED_PATH)
        x = ops.dropout(y1.reshape(T * B, H), p)
        xg = ops.linear_2bias(x, self.l2.weight_ih, self.l2.bias_ih, self.l2.bias_hh)
        y2, h2, c2 = ops.lm_lstm_seq(xg.view(T, B, 4 * H), self.l2.weight_hh, h2, c2, composed=COMPOSED_PATH)
        x = ops.dropout(y2.reshape(T * B, H), p)
        return {'c1': c1, 'h1': h1, 'c2': c2, 'h2': h2}, x

    def forward_seq(self, state, xs):
        """``xs`` (T, B) labels, ``state`` as in ``forward`` -> (state after the window, logits (T, B, V)), differentiable."""
        state, hid = self.window(state, xs)
        T, B = int(xs.shape[0]), int(xs.shape[1])
        return state, ops.linear(hid, self.lo.weight, self.lo.bias).view(T, B, self.n_vocab)

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
    """lm.py:26-109: ``predict(state, x) -> (state, log_probs (n, V))`` for decoding, ``forward(state, x, t) -> (state, loss)`` and
    ``forward_seq(state, xs, ts)`` for training.  Its parameters are ``predictor.*``, so a checkpoint the reference wrote loads with a
    strict ``load_state_dict`` and the other way round."""
    compute_accuracy = True

    def __init__(self, predictor, lossfun=None, accfun=None, label_key=-1):
        if not isinstance(label_key, (int, str)):
            raise TypeError('label_key must be int or str, but is %s' % type(label_key))
        super(ClassifierWithState, self).__init__()
        self.lossfun, self.accfun, self.label_key = lossfun, accfun, label_key
        self.y, self.loss, self.accuracy = None, None, None
        self.predictor = predictor

    def _labels(self, t, dev):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.to(device=dev, dtype=torch.int32).contiguous().view(-1)
        return host_to_dev(np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, np.int32).reshape(-1), dev)

    def forward(self, state, *args, **kwargs):
        """The reference's contract: the argument at ``label_key`` is the labels, the others go to the predictor -> (state, loss), loss
        = mean cross-entropy over the rows (0-dim); sets ``y``, ``loss`` and, with ``compute_accuracy``, ``accuracy``."""
        if isinstance(self.label_key, int):
            if not (-len(args) <= self.label_key < len(args)):
                raise ValueError('Label key %d is out of bounds' % self.label_key)
            t = args[self.label_key]
            args = args[:-1] if self.label_key == -1 else args[:self.label_key] + args[self.label_key + 1:]
        else:
            if self.label_key not in kwargs:
                raise ValueError('Label key "%s" is not found' % self.label_key)
            t = kwargs.pop(self.label_key)
        self.y, self.loss, self.accuracy = None, None, None
        state, self.y = self.predictor(state, *args, **kwargs)
        if self.lossfun is not None:
            self.loss = self.lossfun(self.y, t)
            if self.compute_accuracy and self.accfun is not None:
                self.accuracy = self.accfun(self.y, t)
            return state, self.loss
        loss, stats = ops.cross_entropy(self.y, self._labels(t, self.y.device))
        self.loss = loss.reshape(())
        if self.compute_accuracy:
            self.accuracy = stats[1] / stats[2]
        return state, self.loss

    def forward_seq(self, state, xs, ts):
        """One window: ``xs``, ``ts`` (T, B) labels and targets -> (state, sum over t of the mean cross-entropy of step t), what the
        reference's loop over T ``forward`` calls sums up.  The output layer and the loss run over blocks of whole rows when T*B*V
        would pass OUTPUT_MAX_ELEMS; a block of R rows contributes its mean x R / B, so the total is the same sum over rows / B."""
        rnn = self.predictor
        lo = rnn.lo if isinstance(rnn, RNNLM) else rnn.out          # (model/fsrnn.py FSRNNLM names its output layer ``out``)
        state, hid = rnn.window(state, xs)
        T, B = int(xs.shape[0]), int(xs.shape[1])
        V, rows = rnn.n_vocab, T * B
        tgt = self._labels(ts, hid.device)
        if tgt.numel() != rows:
            raise Re2eError('forward_seq: %d targets for %d x %d labels' % (tgt.numel(), T, B))
        self.y, self.loss, self.accuracy = None, None, None
        block = rows if rows * V <= OUTPUT_MAX_ELEMS else max(1, OUTPUT_MAX_ELEMS // V)
        total, correct = None, None
        for r0 in range(0, rows, block):
            r1 = min(rows, r0 + block)
            logits = ops.linear(hid[r0:r1], lo.weight, lo.bias)
            loss, stats = ops.cross_entropy(logits, tgt[r0:r1], scale=(r1 - r0) / float(B))
            total = loss if total is None else total + loss
            correct = stats[1] if correct is None else correct + stats[1]
            if block == rows:
                self.y = logits.view(T, B, V)
        self.loss = total.reshape(())
        if self.compute_accuracy:
            self.accuracy = correct / rows
        return state, self.loss

    def predict(self, state, x, labels=None):
        state, lp, _ = self.predict_combined(state, x, labels=labels)
        return state, lp

    def predict_combined(self, state, x, att=None, lm_weight=0.0, labels=None):
        """``predict`` plus, when ``att`` (n, V) is given, ``att + lm_weight * log_probs`` (the shallow-fusion score of
        e2e_decoder.py:272, product and sum each rounded to fp32) from the same pass over the rows: (state, log_probs, combined).
        ``labels``: the labels of ``x`` as a host array, for the predictors that branch on them (``host_labels``: model/extlm.py)."""
        if hasattr(self.predictor, 'forward_combined'):          # model/ngram.py NgramLM: the sum comes out of the step's own launch
            return self.predictor.forward_combined(state, x, att, lm_weight)
        if labels is not None and getattr(self.predictor, 'host_labels', False):
            state, z = self.predictor(state, x, labels=labels)
        else:
            state, z = self.predictor(state, x)
        if getattr(self.predictor, 'normalized', False):
            return state, z, (att + float(np.float32(lm_weight)) * z if att is not None else None)
        n, V = z.shape
        lp = _empty(n, V, device=z.device)
        if COMPOSED_PATH or not (isinstance(self.predictor, RNNLM) or getattr(self.predictor, 'fused_combine', False)):
            call('re2e_log_softmax_rows', z.data_ptr(), n, V, V, lp.data_ptr())
            return state, lp, (att + float(np.float32(lm_weight)) * lp if att is not None else None)
        comb = _empty(n, V, device=z.device) if att is not None else None
        call('re2e_lm_log_softmax_combine', z.data_ptr(), n, V, ptr(att), float(np.float32(lm_weight)), lp.data_ptr(), ptr(comb))
        return state, lp, comb


# ---- training (lm.py:148-340, lm_train.py) -----------------------------------------------------------------------------------------------------
def evaluate(model, iter, bproplen=100):
    """Perplexity exp(sum of the per-step losses / steps) over one pass of a ``repeat=False`` iterator, in evaluation mode and without
    gradients, step by step as the reference does (lm.py:240-272); leaves the predictor in training mode."""
    rnn = model.predictor
    rnn.eval()
    state, total, count = None, None, 0
    with torch.no_grad():
        while True:
            try:
                batch = np.asarray(iter.__next__(), np.int32)
            except StopIteration:
                break
            state, loss = model(state, batch[:, 0], batch[:, 1])
            total = loss if total is None else total + loss
            if count % bproplen == 0:
                state = {k: v.detach() for k, v in state.items()}
            count += 1
    rnn.train()
    return float(np.exp(float(total) / count))


def _read_ids(path, char_list_dict):
    with open(path, 'rb') as f:
        return np.array([char_list_dict[c] if c in char_list_dict else char_list_dict['<unk>'] for c in f.readline().decode('utf-8').split()], dtype=np.int32)


def _embed_vecs(path, n_vocab, char_list_dict):
    word_dim = 0
    with open(path, 'r', encoding='utf-8') as fid:
        for line in fid:
            word_dim = len(line.strip().split()[1:])
            break
    vecs = np.array(np.random.uniform(low=-0.05, high=0.05, size=(n_vocab, word_dim)), dtype=np.float32)
    with open(path, 'r', encoding='utf-8') as fid:
        for line in fid:
            parts = line.strip().split()
            if parts and parts[0] in char_list_dict and len(parts) == word_dim + 1:
                vecs[char_list_dict[parts[0]]] = np.array([float(v) for v in parts[1:]], dtype=np.float32)
    return vecs


def train(args):
    """The reference's training loop (lm.py:148-340) over whole windows: every iteration takes ``bproplen`` steps of the training
    iterator as one (T, B) window, sums the per-step losses (forward_seq), back-propagates, detaches the state, clips at ``gradclip``
    and takes an SGD step of lr 1.0; training perplexity every 100 iterations; at each epoch boundary the validation perplexity,
    rnnlm.model.<epoch>, rnnlm.state.<epoch> and the rnnlm.model.best link.  Returns the last validation perplexity (None: no epoch ended)."""
    from ..data.lm_data_loader import ParallelSequentialIterator
    from ..optim import FlatOptimizer
    if args.lm_type != 'rnnlm':
        raise Re2eError('--lm-type %s: only rnnlm is trained here (the FS-RNN LM is trained by model/fsrnn.py train)' % args.lm_type)
    if args.ngpu > 1:
        raise Re2eError('--ngpu %d: the LM trains on one GPU' % args.ngpu)
    if args.ngpu < 1 or not torch.cuda.is_available():
        raise Re2eError('the LM trains on the GPU only (--ngpu 1): there is no CPU path')
    torch.manual_seed(args.seed)
    ops.dropout_seed(args.seed)
    train_ids = _read_ids(args.train_label, args.char_list_dict)
    valid_ids = _read_ids(args.valid_label, args.char_list_dict)
    logging.info('vocabulary: %d', args.n_vocab)
    logging.info('training tokens: %d', len(train_ids))
    logging.info('validation tokens: %d', len(valid_ids))
    logging.info('windows per epoch: %d', len(train_ids) // (args.batchsize * args.bproplen))
    train_iter = ParallelSequentialIterator(train_ids, args.batchsize)
    valid_iter = ParallelSequentialIterator(valid_ids, args.batchsize, repeat=False)
    embed_vecs_init = None
    if getattr(args, 'embed_init_file', None):
        embed_vecs_init = _embed_vecs(args.embed_init_file, args.n_vocab, args.char_list_dict)
        args.input_unit = embed_vecs_init.shape[1]
    model = ClassifierWithState(RNNLM(args.n_vocab, args.input_unit, args.unit, args.dropout_rate, embed_vecs_init))
    model.compute_accuracy = False          # only the perplexity is wanted
    path = os.path.join(args.outdir, 'rnnlm.model.best')
    resumed = os.path.isfile(path)
    if resumed:
        model.load_state_dict(torch.load(path, map_location='cpu'))
        logging.info('resuming from %s', path)
    model.cuda(0)
    model.train()
    optimizer = FlatOptimizer(model.parameters(), kind='sgd', lr=1.0)
    best_valid = evaluate(model, valid_iter) if resumed else 100000000
    sum_perp, count, iteration, epoch_now, state, valid_perp = 0.0, 0, 0, 0, None, None
    while train_iter.epoch < args.epoch:
        iteration += 1
        xs, ts = train_iter.next_window(args.bproplen)
        state, loss = model.forward_seq(state, xs, ts)
        count += args.bproplen
        optimizer.zero_grad()
        loss.backward()
        state = {k: v.detach() for k, v in state.items()}
        optimizer.clip_grad_norm(args.gradclip)
        optimizer.step()
        sum_perp = loss.detach() + sum_perp          # stays on the device: read every 100 iterations
        if iteration % 100 == 0:
            logging.info('iteration %d: training perplexity %.4f', iteration, np.exp(float(sum_perp) / count))
            sum_perp, count = 0.0, 0
        if train_iter.epoch > epoch_now:
            valid_perp = evaluate(model, valid_iter)
            logging.info('epoch %d: validation perplexity %.4f', train_iter.epoch, valid_perp)
            torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, os.path.join(args.outdir, 'rnnlm.model.' + str(epoch_now)))
            torch.save({'state': {}, 'param_groups': [dict(lr=optimizer.param_groups[0]['lr'], momentum=0, dampening=0, weight_decay=0, nesterov=False,
                                                            params=list(range(len(optimizer.params))))]},
                       os.path.join(args.outdir, 'rnnlm.state.' + str(epoch_now)))
            if valid_perp < best_valid:
                dest = os.path.join(args.outdir, 'rnnlm.model.best')
                if os.path.lexists(dest):
                    os.remove(dest)
                os.symlink('rnnlm.model.' + str(epoch_now), dest)
                best_valid = valid_perp
            epoch_now = train_iter.epoch
    return valid_perp
