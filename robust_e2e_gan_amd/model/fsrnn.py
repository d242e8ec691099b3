"""Fast-slow RNN language model (mirror of FSRNNLM, model/fsrnn.py:59-127, trained by lm_train.py --lm-type fsrnnlm and decoded with by
asr_recog.py --lmtype fsrnnlm): decoding and training.

One step is a chain of ``fast_layers`` + 1 LSTM cells, each followed by zoneout:
    x  = d0(embed(ids))
    F  = zo(cell F0(x; F))        S = zo(cell S(d1(F_h); S))        F = zo(cell F1(d2(S_h); F))
    F  = zo(cell Fk(0; F))  for k = 2 .. fast_layers - 1            logits = out(d3(F_h))
with zo(new, old) = m * new + (1 - m) * old: in evaluation mode m = keep (a blend), in training mode every element of m is 1 with
probability keep and 0 otherwise (the reference's Dropout(1 - keep)(ones) * keep is 0, or 1 to within an ulp; here exactly 0 or 1).
fast_cells[1] takes the slow output through an F -> F cell, so the slow cell must be as wide as the fast ones, and fast_layers >= 2
(fsrnn.py:118); both are refused otherwise.  ``LayerNorm`` of the reference's file is never used and is not built.

Training.  A window of T steps x B rows is ONE pass, ``FSRNNLM.window``: embedding -> d0 -> fast cell 0's W_ih product of all T*B rows
(ops.linear_2bias) -> the recurrence (ops.fsrnn_seq: csrc/fsrnn.hip, one fused launch per cell and step -- both products, the cell, zoneout
and the dropped second output -- with the masks as operands) -> d3 -> output layer.  The training masks are drawn from the counter-based
stream of ops.dropout in the reference's order of use, each over its whole (T, B, .) tensor: d0, zo(F0).c, zo(F0).h, d1, zo(S).c, zo(S).h,
d2, zo(F1).c, zo(F1).h, ..., d3; a dropout with p = 0 and a zoneout with keep = 1 draw nothing.  ``forward`` in training mode is the
window with T = 1, so the reference's per-step loop works.

Decoding.  ``forward`` in evaluation mode runs under no_grad: up to 64 rows go through the few-row kernels of csrc/rnnlm.hip
(re2e_lm_lstm_cell_zo once per cell, re2e_lm_output); more rows, or model.lm.COMPOSED_PATH, take the window path with T = 1 (with
COMPOSED_PATH over re2e_gemm + re2e_lstm_cell_fwd + element-wise ops: the tests' arbiter and the timing baseline)."""
import logging
import os

import numpy as np
import torch

from .. import ops
from ..lib import Re2eError, call, ptr
from . import lm as _lm
from .e2e_common import LinearParams, host_to_dev
from .e2e_decoder import EmbeddingParams, LSTMCellParams

STATE_KEYS = ('F_h', 'F_c', 'S_h', 'S_c')


class FSRNNLM(torch.nn.Module):
    """Parameter holder with the reference's state_dict names: embed.weight (V, E), fast_cells.{k}.* (cell 0: E -> F, the others F -> F),
    slow_cell.* (F -> S), out.weight (V, F), out.bias; all initialised uniform(-0.1, 0.1)."""
    fused_combine = True          # ClassifierWithState.predict_combined: raw logits, re2e_lm_log_softmax_combine

    def __init__(self, n_vocab, emb_size, fast_layers, fast_cell_size, slow_cell_size, zoneout_keep_h, zoneout_keep_c, dropout_rate=0.5,
                 embed_vecs_init=None):
        super(FSRNNLM, self).__init__()
        if fast_layers < 2:
            raise Re2eError('FSRNNLM: fast_layers = %d, but the step always runs fast_cells[1] (fsrnn.py:118): at least 2' % fast_layers)
        if slow_cell_size != fast_cell_size:
            raise Re2eError('FSRNNLM: slow_cell_size %d != fast_cell_size %d, but fast_cells[1] takes the slow output through an F -> F cell '
                            '(fsrnn.py:118)' % (slow_cell_size, fast_cell_size))
        if not (0.0 < zoneout_keep_h <= 1.0 and 0.0 < zoneout_keep_c <= 1.0):
            raise Re2eError('FSRNNLM: the zoneout keeps must be in (0, 1]')
        self.n_vocab, self.emb_size, self.dropout_rate, self.fast_layers = n_vocab, emb_size, dropout_rate, fast_layers
        self.F_size, self.S_size = fast_cell_size, slow_cell_size
        self.zoneout_keep_h, self.zoneout_keep_c = zoneout_keep_h, zoneout_keep_c
        self.embed = EmbeddingParams(n_vocab, emb_size)
        self.fast_cells = torch.nn.ModuleList([LSTMCellParams(emb_size, fast_cell_size)] +
                                              [LSTMCellParams(fast_cell_size, fast_cell_size) for _ in range(1, fast_layers)])
        self.slow_cell = LSTMCellParams(fast_cell_size, slow_cell_size)
        self.out = LinearParams(fast_cell_size, n_vocab)
        for param in self.parameters():
            param.data.uniform_(-0.1, 0.1)
        if embed_vecs_init is not None:
            self.embed.weight.data.copy_(torch.from_numpy(np.asarray(embed_vecs_init)))

    def _cells(self):
        return list(self.fast_cells) + [self.slow_cell]

    def _ids(self, x):
        dev = self.out.weight.device
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.to(device=dev, dtype=torch.int32).contiguous().view(-1)
        return host_to_dev(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, np.int32).reshape(-1), dev)

    def _state(self, state, n):
        if state is None:
            return None
        st = tuple(state[k] for k in STATE_KEYS)
        for t in st:
            if tuple(t.shape) != (n, self.F_size):
                raise Re2eError('FSRNNLM state is %s, expected (%d, %d): one row per label in x' % (tuple(t.shape), n, self.F_size))
        return tuple(t.contiguous() for t in st)

    def _need_gpu(self):
        if not self.out.weight.is_cuda:
            raise Re2eError('FSRNNLM parameters are on %s: there is no CPU path (call .cuda())' % self.out.weight.device)

    def forward(self, state, x):
        """``x``: the n last labels; ``state``: {'F_h', 'F_c', 'S_h', 'S_c'} of (n, F) each or None (zeros) -> (state, logits (n, V))."""
        self._need_gpu()
        ids = self._ids(x)
        n = ids.numel()
        if n < 1:
            raise Re2eError('FSRNNLM.forward needs at least one label')
        if self.training:
            state, logits = self.forward_seq(state, ids.view(1, -1))
            return state, logits[0]
        with torch.no_grad():
            if _lm.COMPOSED_PATH or n > _lm.FUSED_MAX_ROWS:
                state, logits = self.forward_seq(state, ids.view(1, -1))
                return state, logits[0]
            return self._forward_fused(self._state(state, n), ids, n)

    def _masks(self, T, B):
        """The training masks of one window behind d0, in the reference's order of use: (mh, mc (L+1,T,B,H) or None, dm (2,T,B,H) or None)."""
        L, H, p = self.fast_layers, self.F_size, self.dropout_rate
        kh, kc = self.zoneout_keep_h, self.zoneout_keep_c
        dev = self.out.weight.device
        with torch.no_grad():
            ones = torch.ones(T, B, H, device=dev)
            mh = torch.empty(L + 1, T, B, H, device=dev) if kh < 1.0 else None
            mc = torch.empty(L + 1, T, B, H, device=dev) if kc < 1.0 else None
            dm = torch.empty(2, T, B, H, device=dev) if p else None
            for c in [0, L] + list(range(1, L)):
                if mc is not None:
                    mc[c].copy_(ops.dropout(ones, 1.0 - kc) != 0)
                if mh is not None:
                    mh[c].copy_(ops.dropout(ones, 1.0 - kh) != 0)
                if dm is not None and c in (0, L):
                    dm[0 if c == 0 else 1].copy_(ops.dropout(ones, p))
        return mh, mc, dm

    def window(self, state, xs):
        """One truncated-BPTT window up to the output layer: ``xs`` (T, B) labels -> (state, hidden (T*B, F) after the last dropout).
        Differentiable in both modes; ``state`` carries autograd history: detach it between windows (the trainer does)."""
        self._need_gpu()
        if not hasattr(xs, 'shape') or len(xs.shape) != 2 or xs.shape[0] < 1 or xs.shape[1] < 1:
            raise Re2eError('FSRNNLM.forward_seq takes labels of shape (T, B)')
        T, B = int(xs.shape[0]), int(xs.shape[1])
        ids = self._ids(xs)
        L, H = self.fast_layers, self.F_size
        st = self._state(state, B)
        if st is None:
            st = (torch.zeros(B, H, device=ids.device),) * 4
        p = self.dropout_rate if self.training else 0.0
        f0 = self.fast_cells[0]
        x = ops.dropout(ops.embedding(self.embed.weight, ids), p)
        xg = ops.linear_2bias(x, f0.weight_ih, f0.bias_ih, f0.bias_hh)
        mh, mc, dm = self._masks(T, B) if self.training else (None, None, None)
        weights = [(c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh) for c in self._cells()]
        y, Fh, Fc, Sh, Sc = ops.fsrnn_seq(xg.view(T, B, 4 * H), st, weights, L, mh=mh, mc=mc, dm=dm,
                                          keep_h=self.zoneout_keep_h if mh is None else 1.0, keep_c=self.zoneout_keep_c if mc is None else 1.0,
                                          composed=_lm.COMPOSED_PATH)
        return {'F_h': Fh, 'F_c': Fc, 'S_h': Sh, 'S_c': Sc}, ops.dropout(y.reshape(T * B, H), p)

    def forward_seq(self, state, xs):
        """``xs`` (T, B) labels, ``state`` as in ``forward`` -> (state after the window, logits (T, B, V)), differentiable."""
        state, hid = self.window(state, xs)
        T, B = int(xs.shape[0]), int(xs.shape[1])
        return state, ops.linear(hid, self.out.weight, self.out.bias).view(T, B, self.n_vocab)

    def _forward_fused(self, st, ids, n):
        dev, V, E, H, L = ids.device, self.n_vocab, self.emb_size, self.F_size, self.fast_layers
        Fh, Fc, Sh, Sc = st if st is not None else (None,) * 4
        kh, kc = float(self.zoneout_keep_h), float(self.zoneout_keep_c)
        fast = _lm._empty(L, 2, n, H, device=dev)               # (h, c) after every fast cell
        slow = _lm._empty(2, n, H, device=dev)

        def cell(c, x, ldx, ids_ptr, n_embed, I, h, cc, out):
            call('re2e_lm_lstm_cell_zo', x, ldx, ids_ptr, n_embed, I, ptr(c.weight_ih) if x is not None else None, ptr(c.weight_hh), ptr(c.bias_ih),
                 ptr(c.bias_hh), ptr(h), ptr(cc), n, H, kh, kc, out[0].data_ptr(), out[1].data_ptr())
        cell(self.fast_cells[0], ptr(self.embed.weight), E, ids.data_ptr(), V, E, Fh, Fc, fast[0])
        cell(self.slow_cell, fast[0, 0].data_ptr(), H, None, 0, H, Sh, Sc, slow)
        cell(self.fast_cells[1], slow[0].data_ptr(), H, None, 0, H, fast[0, 0], fast[0, 1], fast[1])
        for k in range(2, L):
            cell(self.fast_cells[k], None, 0, None, 0, 0, fast[k - 1, 0], fast[k - 1, 1], fast[k])
        logits = _lm._empty(n, V, device=dev)
        call('re2e_lm_output', fast[L - 1, 0].data_ptr(), ptr(self.out.weight), ptr(self.out.bias), n, V, H, logits.data_ptr())
        return {'F_h': fast[L - 1, 0], 'F_c': fast[L - 1, 1], 'S_h': slow[0], 'S_c': slow[1]}, logits


def train(args):
    """The reference's training loop (lm.py:148-340 with --lm-type fsrnnlm) over whole windows, as model.lm.train runs it for the RNNLM:
    forward_seq, backward, detach, clip at ``gradclip``, SGD of lr 1.0; at each epoch boundary the validation perplexity,
    rnnlm.model.<epoch>, rnnlm.state.<epoch> and the rnnlm.model.best link.  Returns the last validation perplexity (None: no epoch ended)."""
    from ..data.lm_data_loader import ParallelSequentialIterator
    from ..optim import FlatOptimizer
    if args.lm_type != 'fsrnnlm':
        raise Re2eError('--lm-type %s: model/fsrnn.py trains the FS-RNN LM (fsrnnlm) only' % args.lm_type)
    if args.ngpu > 1:
        raise Re2eError('--ngpu %d: the LM trains on one GPU' % args.ngpu)
    if args.ngpu < 1 or not torch.cuda.is_available():
        raise Re2eError('the LM trains on the GPU only (--ngpu 1): there is no CPU path')
    torch.manual_seed(args.seed)
    ops.dropout_seed(args.seed)
    train_ids = _lm._read_ids(args.train_label, args.char_list_dict)
    valid_ids = _lm._read_ids(args.valid_label, args.char_list_dict)
    logging.info('vocabulary: %d', args.n_vocab)
    logging.info('training tokens: %d', len(train_ids))
    logging.info('validation tokens: %d', len(valid_ids))
    train_iter = ParallelSequentialIterator(train_ids, args.batchsize)
    valid_iter = ParallelSequentialIterator(valid_ids, args.batchsize, repeat=False)
    embed_vecs_init = None
    if getattr(args, 'embed_init_file', None):
        embed_vecs_init = _lm._embed_vecs(args.embed_init_file, args.n_vocab, args.char_list_dict)
        args.input_unit = embed_vecs_init.shape[1]
    model = _lm.ClassifierWithState(FSRNNLM(args.n_vocab, args.input_unit, args.fast_layers, args.fast_cell_size, args.slow_cell_size,
                                            args.zoneout_keep_h, args.zoneout_keep_c, args.dropout_rate, embed_vecs_init))
    model.compute_accuracy = False          # only the perplexity is wanted
    path = os.path.join(args.outdir, 'rnnlm.model.best')
    resumed = os.path.isfile(path)
    if resumed:
        model.load_state_dict(torch.load(path, map_location='cpu'))
        logging.info('resuming from %s', path)
    model.cuda(0)
    model.train()
    optimizer = FlatOptimizer(model.parameters(), kind='sgd', lr=1.0)
    best_valid = _lm.evaluate(model, valid_iter) if resumed else 100000000
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
            valid_perp = _lm.evaluate(model, valid_iter)
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
