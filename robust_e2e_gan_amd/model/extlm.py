"""Word-level language models for decoding (mirror of LookAheadWordLM / MultiLevelLM, model/extlm.py:75-216), decode side only.

A character-level beam search scores words with a word RNNLM through a lexical tree (Hori et al., "End-to-end speech recognition with
word-based RNN language models"): LookAheadWordLM gives every character the word LM's mass of the words that continue the prefix;
MultiLevelLM scores characters with a character RNNLM and swaps in the word LM's score at word ends.  Upstream both run one hypothesis
per call over a nested dict tree, with a softmax and cumsum over the word vocabulary and a Python loop over a node's children.  Here all
``n`` live hypotheses of a position go through ONE ``forward``:

* the tree is flattened once into int32 arrays (``LexicalTree``) and lives on the device; a hypothesis holds a node id (-1 = upstream's
  ``None``: no path in the tree, open-vocabulary mode);
* the state is a dict of tensors whose dimension 0 is the row, so the searches' ``index_select(0, parents)`` carries it:
  LookAheadWordLM  c1, h1, c2, h2 (n, H) of the word LM, cumsum (n, Vw) fp32, node (n,) int32;
  MultiLevelLM     the same four, sub_c1 .. sub_h2 of the character LM, wlm_logprobs (n, Vw), log_y (n, Vc), clm_logprob (n,), node;
* the word LM advances ONLY for the rows whose label is <space>: they are gathered, go through RNNLM.forward (few-row kernels) and are
  scattered back; with no row at a space neither the word LM nor the scan runs.  The searches hand down the labels they hold on the host
  (``labels=``), so knowing which rows those are costs no device->host copy; without them ``x`` is read back once;
* csrc/wordlm.hip does the rest: re2e_wlm_transition, re2e_wlm_softmax_cumsum (running sums in fp64), re2e_wlm_lookahead,
  re2e_wlm_multilevel_fix.  ``forward`` never modifies its input state (unchanged tensors are shared between the old and the new one).

``ARBITER_PATH`` swaps in the same predictors over torch ops on device tensors (softmax, cumsum, log_softmax) with a per-row Python walk
of the flat tree: the tests' arbiter and the timing baseline (tools/bench_recog_wordlm.py), not a user option.

NgramCharacterKenLM (extlm.py:46-72 upstream) is model/ngram.py here: ARPA back-off models on kernels of their own.  Out of scope: training."""
import math

import numpy as np
import torch

from ..lib import Re2eError, call
from .e2e_common import host_to_dev
from .lm import RNNLM, STATE_KEYS

ARBITER_PATH = False           # tests / tools: torch ops + a per-row walk of the tree instead of csrc/wordlm.hip (arbiter, timing baseline)
SUB_KEYS = tuple('sub_' + k for k in STATE_KEYS)
LOGZERO = -10000000000.0
ZERO = 1.0e-10


def _empty(*shape, **kw):
    """Every output buffer of a step comes from here (tests hand out NaN-filled ones: a kernel must write all of it)."""
    return torch.empty(*shape, **kw)


class LexicalTree(object):
    """The prefix tree of the words a character sequence can spell (make_lexical_tree, extlm.py:21-42), as flat int32 arrays.  Included: every
    word with id > 0 other than ``word_unk`` whose characters are all in ``subword_dict``.  Node 0 is the root; ``wid[k]`` is the word that
    ends at node k or -1; (``lo[k]``, ``hi[k]``) = (smallest word id below the node - 1, largest word id), so that the node's word mass is
    ``cumsum[hi] - cumsum[lo]`` (the root carries lo = hi = -1: mass 1); the children of node k are entries ``child_off[k]`` ..
    ``child_off[k + 1] - 1`` of ``child_label`` / ``child_node``, labels ascending.  Nodes are numbered breadth first."""

    def __init__(self, word_dict, subword_dict, word_unk):
        kids, wid, lo, hi = [{}], [-1], [-1], [-1]                # grown node by node
        for word, w in word_dict.items():
            if w <= 0 or w == word_unk or any(ch not in subword_dict for ch in word):
                continue
            k = 0
            for pos, ch in enumerate(word):
                label = subword_dict[ch]
                nxt = kids[k].get(label)
                if nxt is None:
                    nxt = len(kids)
                    kids[k][label] = nxt
                    kids.append({}), wid.append(-1), lo.append(w - 1), hi.append(w)
                else:
                    lo[nxt], hi[nxt] = min(lo[nxt], w - 1), max(hi[nxt], w)
                if pos == len(word) - 1:
                    wid[nxt] = w
                k = nxt
        order, at = [0], 0                                          # breadth first, labels ascending
        while at < len(order):
            order.extend(kids[order[at]][label] for label in sorted(kids[order[at]]))
            at += 1
        new_id = {old: new for new, old in enumerate(order)}
        N = len(order)
        self.n_nodes = N
        self.wid = np.asarray([wid[o] for o in order], np.int32)
        self.lo = np.asarray([lo[o] for o in order], np.int32)
        self.hi = np.asarray([hi[o] for o in order], np.int32)
        self.child_off = np.zeros(N + 1, np.int32)
        labels, nodes = [], []
        for new, old in enumerate(order):
            for label in sorted(kids[old]):
                labels.append(label)
                nodes.append(new_id[kids[old][label]])
            self.child_off[new + 1] = len(labels)
        self.child_label, self.child_node = np.asarray(labels, np.int32).reshape(-1), np.asarray(nodes, np.int32).reshape(-1)
        self.n_children = len(labels)
        self.max_wid = int(self.hi.max()) if N > 1 else -1
        self._dev = {}

    ARRAYS = ('wid', 'lo', 'hi', 'child_off', 'child_label', 'child_node')

    def children(self, k):
        """{label: node} of node k."""
        a, b = int(self.child_off[k]), int(self.child_off[k + 1])
        return dict(zip(self.child_label[a:b].tolist(), self.child_node[a:b].tolist()))

    def step(self, k, label):
        """The child of node k (-1: none) with this label, or -1."""
        if k < 0:
            return -1
        a, b = int(self.child_off[k]), int(self.child_off[k + 1])
        j = a + int(np.searchsorted(self.child_label[a:b], label))
        return int(self.child_node[j]) if j < b and self.child_label[j] == label else -1

    def dev(self, device):
        """The arrays on ``device``, uploaded once (an empty child list is one padding entry, so that every array has an address)."""
        key = str(device)
        if key not in self._dev:
            pad = lambda a: a if a.size else np.full(1, -1, np.int32)
            self._dev[key] = {name: torch.from_numpy(pad(getattr(self, name))).to(device) for name in self.ARRAYS}
        return self._dev[key]


class _WordLevelLM(torch.nn.Module):
    """What the two models share: the dictionaries' special ids, the tree, the word LM's advance at the rows that stand at a <space>."""
    logzero = LOGZERO
    zero = ZERO
    normalized = True            # forward returns log-probabilities (ClassifierWithState.predict_combined)
    host_labels = True           # forward takes the labels the caller holds on the host (labels=)

    def _setup(self, wordlm, word_dict, subword_dict, open_vocab):
        for name in ('<eos>', '<unk>'):
            if name not in word_dict:
                raise KeyError('word_dict has no %s' % name)
        for name in ('<space>', '<eos>'):
            if name not in subword_dict:
                raise KeyError('subword_dict has no %s' % name)
        if not isinstance(wordlm, RNNLM):
            raise Re2eError('wordlm must be a model.lm.RNNLM, got %s' % type(wordlm).__name__)
        self.wordlm = wordlm
        self.word_eos, self.word_unk = int(word_dict['<eos>']), int(word_dict['<unk>'])
        self.space, self.eos = int(subword_dict['<space>']), int(subword_dict['<eos>'])
        self.subword_dict_size = len(subword_dict)
        self.open_vocab = bool(open_vocab)
        self.tree = LexicalTree(word_dict, subword_dict, self.word_unk)
        Vw = wordlm.n_vocab
        # cumsum[word - 1] is read for <unk>, <eos> and every word end: ids 1 .. Vw - 1 (upstream id 0 would wrap round to the last column)
        if not (1 <= self.word_unk < Vw and 1 <= self.word_eos < Vw and self.tree.max_wid < Vw):
            raise Re2eError('word ids must lie in [1, %d): <unk> = %d, <eos> = %d, largest word id in the tree = %d'
                            % (Vw, self.word_unk, self.word_eos, self.tree.max_wid))
        if not (0 <= self.space < self.subword_dict_size and 0 <= self.eos < self.subword_dict_size):
            raise Re2eError('<space> = %d / <eos> = %d outside the %d subword labels' % (self.space, self.eos, self.subword_dict_size))

    @property
    def device(self):
        return self.wordlm.lo.weight.device

    def _rows(self, x, labels):
        ids = self.wordlm._ids(x)
        n = ids.numel()
        if n < 1:
            raise Re2eError('%s.forward needs at least one label' % type(self).__name__)
        host = ids.cpu().numpy() if labels is None else np.asarray(labels, np.int64).reshape(-1)     # without labels=: one small read-back
        if host.shape[0] != n:
            raise Re2eError('labels has %d entries, x has %d' % (host.shape[0], n))
        return ids, host, n

    def _check_state(self, state, n, keys):
        for k in keys:
            if k not in state or state[k].shape[0] != n:
                raise Re2eError('%s state: %r is %s, expected %d rows: one per label in x'
                                % (type(self).__name__, k, tuple(state[k].shape) if k in state else None, n))

    def _initial_word(self, n):
        """The word LM fed <eos>, once, for all n rows: (state of (n, H) tensors, logits (1, Vw))."""
        st, z = self.wordlm(None, np.asarray([self.word_eos], np.int32))
        return {k: v.expand(n, -1).contiguous() for k, v in st.items()}, z

    def _advance_word(self, state, word_in, sp_rows, n):
        """The word LM's step for the rows ``sp_rows`` (host, ascending) fed ``word_in[rows]``: (the n-row state with those rows replaced --
        fresh tensors --, logits (m, Vw), the rows as int32 / int64 device tensors or None when they are all n rows)."""
        m = len(sp_rows)
        if m == n:
            new, z = self.wordlm({k: state[k] for k in STATE_KEYS}, word_in)
            return new, z, None, None
        rows = host_to_dev(np.asarray(sp_rows, np.int64), self.device, torch.int64)
        new, z = self.wordlm({k: state[k].index_select(0, rows) for k in STATE_KEYS}, word_in.index_select(0, rows))
        return {k: state[k].clone().index_copy_(0, rows, new[k]) for k in STATE_KEYS}, z, rows.to(torch.int32), rows

    def _transition(self, state, ids, host, n):
        """re2e_wlm_transition for the n rows: (node_new, word_in, at_space) int32 device tensors and the host rows that stand at a <space>."""
        t = self.tree.dev(self.device)
        out = _empty(3, n, dtype=torch.int32, device=self.device)
        node = state['node'].to(torch.int32).contiguous()
        call('re2e_wlm_transition', node.data_ptr(), ids.data_ptr(), n, self.subword_dict_size, self.space, self.word_unk, t['wid'].data_ptr(),
             t['child_off'].data_ptr(), t['child_label'].data_ptr(), t['child_node'].data_ptr(), self.tree.n_nodes, self.tree.n_children,
             out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
        return out[0], out[1], out[2], np.nonzero(host == self.space)[0]

    def _walk(self, state, host):
        """The arbiter's transition: per row (new node, word id for the word LM, at-space flag) on the host."""
        prev = state['node'].cpu().tolist()
        N, tree = self.tree.n_nodes, self.tree
        nodes, words, flags = [], [], []
        for nd, x in zip(prev, host.tolist()):
            if not (0 <= x < self.subword_dict_size and -1 <= nd < N):
                nodes.append(-1), words.append(self.word_unk), flags.append(-1)
            elif x == self.space:
                nodes.append(0), words.append(int(tree.wid[nd]) if nd >= 0 and tree.wid[nd] >= 0 else self.word_unk), flags.append(1)
            else:
                nodes.append(tree.step(nd, x)), words.append(self.word_unk), flags.append(0)
        return nodes, words, flags

    def _guard(self):
        if self.training:
            raise Re2eError('%s runs in evaluation mode only (call .eval())' % type(self).__name__)


class LookAheadWordLM(_WordLevelLM):
    """extlm.py:149-216: a word RNNLM alone.  P(c | prefix) = the word LM's mass of the words below the child node over the mass below the
    node; at a word end <space> gets the word's own probability and <eos> that times P(<eos>); labels off the tree get
    P(<unk>) * oov_penalty, and a hypothesis that has left the tree scores log 1 (or ``logzero`` with ``open_vocab`` off) until the next
    <space> feeds <unk> to the word LM."""

    def __init__(self, wordlm, word_dict, subword_dict, oov_penalty=0.0001, open_vocab=True):
        super(LookAheadWordLM, self).__init__()
        self._setup(wordlm, word_dict, subword_dict, open_vocab)
        self.oov_penalty = oov_penalty

    def forward(self, state, x, labels=None):
        """``x``: the n last labels; ``state``: None or {'c1', 'h1', 'c2', 'h2', 'cumsum', 'node'}; ``labels``: the same labels on the host.
        Returns (state, log-probabilities (n, subword_dict_size))."""
        self._guard()
        with torch.no_grad():
            ids, host, n = self._rows(x, labels)
            if state is not None:
                self._check_state(state, n, STATE_KEYS + ('cumsum', 'node'))
            if ARBITER_PATH:
                return self._forward_arbiter(state, host, n)
            dev, Vw, Vc = self.device, self.wordlm.n_vocab, self.subword_dict_size
            if state is None:
                wst, z = self._initial_word(n)
                first = _empty(1, Vw, device=dev)
                call('re2e_wlm_softmax_cumsum', z.data_ptr(), 1, Vw, None, 1, first.data_ptr())
                cumsum = first.expand(n, Vw).contiguous()
                node, at = torch.zeros(n, dtype=torch.int32, device=dev), torch.ones(n, dtype=torch.int32, device=dev)
            else:
                node, word_in, at, sp_rows = self._transition(state, ids, host, n)
                wst, cumsum = {k: state[k] for k in STATE_KEYS}, state['cumsum'].contiguous()
                if len(sp_rows):
                    wst, z, rows32, _ = self._advance_word(state, word_in, sp_rows, n)
                    cumsum = _empty(n, Vw, device=dev) if rows32 is None else cumsum.clone()
                    call('re2e_wlm_softmax_cumsum', z.data_ptr(), len(sp_rows), Vw, rows32.data_ptr() if rows32 is not None else None, n,
                         cumsum.data_ptr())
            t = self.tree.dev(dev)
            log_y = _empty(n, Vc, device=dev)
            call('re2e_wlm_lookahead', cumsum.data_ptr(), n, Vw, node.data_ptr(), at.data_ptr(), t['wid'].data_ptr(), t['lo'].data_ptr(),
                 t['hi'].data_ptr(), t['child_off'].data_ptr(), t['child_label'].data_ptr(), t['child_node'].data_ptr(), self.tree.n_nodes,
                 self.tree.n_children, Vc, self.space, self.eos, self.word_unk, self.word_eos, float(np.float32(self.oov_penalty)),
                 int(self.open_vocab), log_y.data_ptr())
            return dict(wst, cumsum=cumsum, node=node), log_y

    def _forward_arbiter(self, state, host, n):
        dev, Vc, tree = self.device, self.subword_dict_size, self.tree
        if state is None:
            wst, z = self._initial_word(n)
            cumsum = torch.cumsum(torch.softmax(z, dim=1), dim=1).expand(n, -1).contiguous()
            nodes, flags = [0] * n, [1] * n
        else:
            nodes, words, flags = self._walk(state, host)
            wst, cumsum = {k: state[k] for k in STATE_KEYS}, state['cumsum']
            sp_rows = np.asarray([r for r in range(n) if flags[r] == 1 or (flags[r] == -1 and host[r] == self.space)], np.int64)
            if len(sp_rows):
                word_in = torch.tensor(words, dtype=torch.int32, device=dev)
                wst, z, _, rows = self._advance_word(state, word_in, sp_rows, n)
                cs = torch.cumsum(torch.softmax(z, dim=1), dim=1)
                cumsum = cs if rows is None else cumsum.clone().index_copy_(0, rows, cs)
        out = []
        for r in range(n):
            nd = nodes[r]
            if flags[r] < 0:
                out.append(torch.full((Vc,), float('nan'), device=dev))
                continue
            if nd < 0:
                out.append(torch.zeros(Vc, device=dev) + (0.0 if self.open_vocab else self.logzero))
                continue
            c = cumsum[r]
            sum_prob = (c[int(tree.hi[nd])] - c[int(tree.lo[nd])]) if tree.lo[nd] >= 0 else 1.0
            y = torch.zeros(Vc, device=dev) + (c[self.word_unk] - c[self.word_unk - 1]) * self.oov_penalty
            a, b = int(tree.child_off[nd]), int(tree.child_off[nd + 1])
            if b > a:
                kids = tree.child_node[a:b]
                idx = torch.from_numpy(np.stack([tree.child_label[a:b], tree.hi[kids], tree.lo[kids]]).astype(np.int64)).to(dev)
                y[idx[0]] = (c[idx[1]] - c[idx[2]]) / sum_prob
            w = int(tree.wid[nd])
            if w >= 0:
                wlm_prob = (c[w] - c[w - 1]) / sum_prob
                y[self.space] = wlm_prob
                y[self.eos] = wlm_prob * (c[self.word_eos] - c[self.word_eos - 1])
            elif flags[r] == 1:
                y[self.space] = self.zero
                y[self.eos] = self.zero
            out.append(torch.log(y))
        return dict(wst, cumsum=cumsum, node=torch.tensor(nodes, dtype=torch.int32, device=dev)), torch.stack(out)


class MultiLevelLM(_WordLevelLM):
    """extlm.py:75-145: a character RNNLM inside words (weighted by ``subwordlm_weight``), the word RNNLM at word ends: <space> scores the word's
    log-probability minus what the character LM has already given its letters (or log P(<unk>) + log oov_penalty off the tree), <eos> that plus
    log P(<eos>)."""

    def __init__(self, wordlm, subwordlm, word_dict, subword_dict, subwordlm_weight=0.8, oov_penalty=1.0, open_vocab=True):
        super(MultiLevelLM, self).__init__()
        self._setup(wordlm, word_dict, subword_dict, open_vocab)
        if not isinstance(subwordlm, RNNLM):
            raise Re2eError('subwordlm must be a model.lm.RNNLM, got %s' % type(subwordlm).__name__)
        if subwordlm.n_vocab != self.subword_dict_size:
            raise Re2eError('subwordlm has %d labels, subword_dict %d' % (subwordlm.n_vocab, self.subword_dict_size))
        self.subwordlm = subwordlm
        self.log_oov_penalty = math.log(oov_penalty)
        self.subwordlm_weight = subwordlm_weight

    KEYS = STATE_KEYS + SUB_KEYS + ('wlm_logprobs', 'log_y', 'clm_logprob', 'node')

    def _sub_step(self, state, ids, dead):
        """The character LM's step for all rows; ``dead`` rows (no path, open_vocab off: upstream returns before this step) keep their state."""
        old = None if state is None else dict(zip(STATE_KEYS, (state[k] for k in SUB_KEYS)))
        new, z = self.subwordlm(old, ids)
        if dead is not None:
            new = {k: torch.where(dead[:, None], old[k], new[k]) for k in STATE_KEYS}
        return dict(zip(SUB_KEYS, (new[k] for k in STATE_KEYS))), z

    def forward(self, state, x, labels=None):
        """``x``: the n last labels; ``state``: None or the dict of ``KEYS``; ``labels``: the same labels on the host.  Returns (state,
        log-probabilities (n, subword_dict_size))."""
        self._guard()
        with torch.no_grad():
            ids, host, n = self._rows(x, labels)
            if state is not None:
                self._check_state(state, n, self.KEYS)
            if ARBITER_PATH:
                return self._forward_arbiter(state, ids, host, n)
            dev, Vw, Vc = self.device, self.wordlm.n_vocab, self.subword_dict_size
            if state is None:
                wst, z = self._initial_word(n)
                first = _empty(1, Vw, device=dev)
                call('re2e_lm_log_softmax_combine', z.data_ptr(), 1, Vw, None, 0.0, first.data_ptr(), None)
                wlp = first.expand(n, Vw).contiguous()
                node, at = torch.zeros(n, dtype=torch.int32, device=dev), torch.ones(n, dtype=torch.int32, device=dev)
                sst, zc = self._sub_step(None, ids, None)
                clm_prev = y_prev = None
            else:
                node, word_in, at, sp_rows = self._transition(state, ids, host, n)
                wst, wlp = {k: state[k] for k in STATE_KEYS}, state['wlm_logprobs'].contiguous()
                if len(sp_rows):
                    wst, z, _, rows = self._advance_word(state, word_in, sp_rows, n)
                    lp = _empty(len(sp_rows), Vw, device=dev)
                    call('re2e_lm_log_softmax_combine', z.data_ptr(), len(sp_rows), Vw, None, 0.0, lp.data_ptr(), None)
                    wlp = lp if rows is None else wlp.clone().index_copy_(0, rows, lp)
                sst, zc = self._sub_step(state, ids, None if self.open_vocab else (node < 0) & (at == 0))
                clm_prev, y_prev = state['clm_logprob'].contiguous(), state['log_y'].contiguous()
            lsm = _empty(n, Vc, device=dev)
            call('re2e_log_softmax_rows', zc.data_ptr(), n, Vc, Vc, lsm.data_ptr())
            log_y, clm = _empty(n, Vc, device=dev), _empty(n, device=dev)
            call('re2e_wlm_multilevel_fix', lsm.data_ptr(), wlp.data_ptr(), n, Vw, node.data_ptr(), at.data_ptr(),
                 self.tree.dev(dev)['wid'].data_ptr(), self.tree.n_nodes, clm_prev.data_ptr() if clm_prev is not None else None,
                 y_prev.data_ptr() if y_prev is not None else None, ids.data_ptr() if clm_prev is not None else None, Vc, self.space, self.eos,
                 self.word_unk, self.word_eos, float(np.float32(self.subwordlm_weight)), float(np.float32(self.log_oov_penalty)),
                 int(self.open_vocab), log_y.data_ptr(), clm.data_ptr())
            return dict(wst, wlm_logprobs=wlp, log_y=log_y, clm_logprob=clm, node=node, **sst), log_y

    def _forward_arbiter(self, state, ids, host, n):
        dev, Vc, tree = self.device, self.subword_dict_size, self.tree
        if state is None:
            wst, z = self._initial_word(n)
            wlp = torch.log_softmax(z, dim=1).expand(n, -1).contiguous()
            nodes, flags = [0] * n, [1] * n
            sst, zc = self._sub_step(None, ids, None)
            clm = torch.zeros(n, device=dev)
        else:
            nodes, words, flags = self._walk(state, host)
            wst, wlp = {k: state[k] for k in STATE_KEYS}, state['wlm_logprobs']
            sp_rows = np.asarray([r for r in range(n) if flags[r] == 1 or (flags[r] == -1 and host[r] == self.space)], np.int64)
            if len(sp_rows):
                word_in = torch.tensor(words, dtype=torch.int32, device=dev)
                wst, z, _, rows = self._advance_word(state, word_in, sp_rows, n)
                lp = torch.log_softmax(z, dim=1)
                wlp = lp if rows is None else wlp.clone().index_copy_(0, rows, lp)
            dead = [flags[r] == 0 and nodes[r] < 0 and not self.open_vocab for r in range(n)]
            sst, zc = self._sub_step(state, ids, None if self.open_vocab else torch.tensor(dead, device=dev))
            walked = state['clm_logprob'] + state['log_y'].gather(1, ids.long().clamp(0, Vc - 1)[:, None])[:, 0]
            clm = torch.where(torch.tensor([f == 0 and not d for f, d in zip(flags, dead)], device=dev), walked, torch.zeros(n, device=dev))
        log_y = torch.log_softmax(zc, dim=1) * self.subwordlm_weight
        for r in range(n):
            if flags[r] < 0:
                log_y[r] = float('nan')
                clm[r] = float('nan')
            elif state is not None and dead[r]:
                log_y[r] = self.logzero
            elif flags[r] == 1:
                log_y[r, self.space] = self.logzero
                log_y[r, self.eos] = self.logzero
            else:
                w = int(tree.wid[nodes[r]]) if nodes[r] >= 0 else -1
                s = wlp[r, w] - clm[r] if w >= 0 else wlp[r, self.word_unk] + self.log_oov_penalty
                log_y[r, self.space] = s
                log_y[r, self.eos] = s + wlp[r, self.word_eos]
        return dict(wst, wlm_logprobs=wlp, log_y=log_y, clm_logprob=clm, node=torch.tensor(nodes, dtype=torch.int32, device=dev), **sst), log_y
