"""N-gram language models for decoding: ARPA back-off models scored on the device (the reference's --kenlm / NgramCharacterKenLM,
model/extlm.py:46-72, utils/kenlm_rescore.py; neither kenlm nor pyfst is used: the ARPA text format and Katz back-off are a definition).

Upstream asks kenlm for one label of one hypothesis at a time on the host and for that reason left the call commented out of its own search
(e2e_decoder.py:263-265).  Here the whole model sits in HBM as flat arrays and one position of the search is one launch (csrc/ngram.hip):

* ``read_arpa`` reads the text format (orders 1 .. 8) and refuses what is not a model with ``ArpaError`` and the line number;
* ``NgramTables`` maps the file's tokens to decoder labels and lays the model out: node 0 is the root, every n-gram of length
  1 .. order - 1 is a node with its back-off ``bo``, the node of its longest proper suffix that is a node (``bo_node``) and a CSR list of
  successors (``succ_off`` / ``succ_label`` ascending / ``succ_logp`` / ``succ_next`` = the node of the longest suffix of context + label that
  is a node); the root's successors are the dense rows ``uni_logp`` / ``uni_next``.  The file may be pruned: suffixes need not exist.  A
  hypothesis holds a node id, and the score of label v after it is the sum of the back-offs of the chain node, bo_node[node], ... down to the
  first level that holds v, plus v's log-probability there -- the dictionary form of Katz back-off, exactly;
* ``NgramLM`` is the predictor the searches drive (``forward(state, x) -> ({'node': (n,) int32}, lp (n, V))``); ``forward_combined`` also
  returns ``att + lm_weight * lp`` from the same launch (ClassifierWithState.predict_combined).

Scores are NATURAL logarithms in the search, where they are added to natural-log attention / CTC scores (values of the file x ln 10, taken in
double and rounded once to fp32).  They are log10 only in the output of the rescoring tool (utils/ngram_rescore.py), as upstream.

Token mapping.  ``tokens='symbols'``: a token of the file is the dictionary's symbol; ``tokens='ids'``: it is the decimal label id (what the
reference's class feeds kenlm: ``str(int(hyp))``).  The decoder starts every hypothesis with the eos label (sos == eos), so in ``symbols`` mode
``<s>`` and ``</s>`` both map to the label eos: the one-label context [eos] carries the log-probability of ``</s>`` and the back-off of ``<s>``;
in ``ids`` mode the token ``str(eos)`` plays both roles, as upstream.  A label whose token has no unigram is the file's ``<unk>`` in every
position, the history included; without an ``<unk>`` such a label scores ``LOGZERO`` = -1e10 and leaves the state at the root.  Tokens of the
file that are no label are dropped with every n-gram that contains them (``tables.dropped`` counts the tokens).

``tables.step_host`` walks the same fp32 arrays with numpy fp32 additions in the kernel's order; ``HOST_PATH`` routes ``NgramLM`` through it:
the tests' arbiter and the timing baseline (tools/bench_recog_ngram.py), not a user option.

Out of scope: an n-gram LM inside MultiLevelLM, an n-gram LM and an RNNLM together, binary KenLM files and FST files (export ARPA), training or
estimating n-gram models, word-level n-grams."""
import math
import os

import numpy as np
import torch

from ..lib import Re2eError, call
from .e2e_common import host_to_dev

MAX_ORDER = 8
LOGZERO = -10000000000.0
LN10 = math.log(10.0)
HOST_PATH = False              # tests / tools: NgramLM over tables.step_host instead of csrc/ngram.hip (arbiter, timing baseline)


class ArpaError(ValueError):
    """What ``read_arpa`` refuses; ``lineno`` is the 1-based line of the file."""

    def __init__(self, lineno, msg):
        super(ArpaError, self).__init__('line %d: %s' % (lineno, msg))
        self.lineno = lineno


def read_arpa(path):
    """``[{(w1, .., wk): (log10 p, log10 back-off)}]`` for k = 1 .. order, tokens as strings, from an ARPA file: the ``\\data\\`` counts, then per
    order a ``\\k-grams:`` section of ``log10p <TAB> w1 .. wk [<TAB> log10 backoff]`` lines, then ``\\end\\``.  Raises ArpaError (with the line)
    for a count that disagrees with its section (at the section's header), an n-gram whose (k-1)-prefix is absent, a duplicate n-gram, a
    back-off on the highest order, an order above 8, an unparsable number and a file without ``\\end\\``."""
    counts, grams, header_line = {}, [], {}
    section, in_data, ended, lineno = 0, False, False, 0

    def number(text, what):
        try:
            v = float(text)
        except ValueError:
            raise ArpaError(lineno, 'cannot parse %s %r' % (what, text))
        if v != v:
            raise ArpaError(lineno, 'cannot parse %s %r' % (what, text))
        return v

    with open(path, 'r', encoding='utf-8') as f:
        for lineno, raw in enumerate(f, 1):
            line = raw.strip()
            if not line:
                continue
            if line == '\\data\\':
                in_data = True
                continue
            if line == '\\end\\':
                ended = True
                break
            if line.startswith('\\') and line.endswith('-grams:'):
                try:
                    k = int(line[1:-len('-grams:')])
                except ValueError:
                    raise ArpaError(lineno, 'cannot parse the section header %r' % line)
                if k > MAX_ORDER:
                    raise ArpaError(lineno, 'order %d: orders 1 .. %d are supported' % (k, MAX_ORDER))
                if k != section + 1 or k not in counts:
                    raise ArpaError(lineno, 'section %r out of place (after order %d; \\data\\ names %s)' % (line, section, sorted(counts)))
                section, in_data = k, False
                header_line[k] = lineno
                grams.append({})
                continue
            if in_data:
                if not line.startswith('ngram ') or '=' not in line:
                    raise ArpaError(lineno, 'expected "ngram K=COUNT", got %r' % line)
                a, b = line[len('ngram '):].split('=', 1)
                try:
                    k, c = int(a), int(b)
                except ValueError:
                    raise ArpaError(lineno, 'cannot parse the count %r' % line)
                if k > MAX_ORDER:
                    raise ArpaError(lineno, 'order %d: orders 1 .. %d are supported' % (k, MAX_ORDER))
                if k < 1 or c < 0 or k in counts:
                    raise ArpaError(lineno, 'bad count line %r' % line)
                counts[k] = c
                continue
            if section == 0:
                continue                                        # text in front of \data\ (a header some tools write)
            fields = line.split()
            if len(fields) not in (section + 1, section + 2):
                raise ArpaError(lineno, 'a %d-gram line has %d or %d fields, got %r' % (section, section + 1, section + 2, line))
            logp = number(fields[0], 'the log-probability')
            words = tuple(fields[1:section + 1])
            bo = 0.0
            if len(fields) == section + 2:
                if section == max(counts):
                    raise ArpaError(lineno, 'a back-off weight on the highest order (%d): %r' % (section, ' '.join(words)))
                bo = number(fields[-1], 'the back-off weight')
            if words in grams[-1]:
                raise ArpaError(lineno, 'duplicate n-gram %r' % ' '.join(words))
            if section > 1 and words[:-1] not in grams[-2]:
                raise ArpaError(lineno, 'n-gram %r: its prefix %r is not in the %d-grams' % (' '.join(words), ' '.join(words[:-1]), section - 1))
            grams[-1][words] = (logp, bo)
    if not ended:
        raise ArpaError(max(lineno, 1), 'no \\end\\: the file is cut short or is not an ARPA file')
    if not counts:
        raise ArpaError(max(lineno, 1), 'no \\data\\ counts')
    for k in sorted(counts):
        if k > len(grams):
            raise ArpaError(lineno, '\\data\\ names order %d but there is no \\%d-grams: section' % (k, k))
        if len(grams[k - 1]) != counts[k]:
            raise ArpaError(header_line[k], '\\data\\ says %d %d-grams, the section has %d' % (counts[k], k, len(grams[k - 1])))
    return grams


def _suffix_node(node_of, g, longest):
    """The node of the longest suffix of ``g`` of at most ``longest`` labels that is a node (the root, 0, for the empty one)."""
    for start in range(max(0, len(g) - longest), len(g)):
        nd = node_of.get(g[start:])
        if nd is not None:
            return nd
    return 0


class NgramTables(object):
    """The flat arrays of one model over V decoder labels (module docstring).  ``ARRAYS`` names them; ``order``, ``n_vocab``, ``eos``,
    ``n_nodes`` (N), ``n_succ``, ``dropped`` (tokens of the file that were no label), ``has_unk`` and ``tokens`` (the mapping mode) go with them."""
    ARRAYS = ('uni_logp', 'uni_next', 'bo', 'bo_node', 'succ_off', 'succ_label', 'succ_logp', 'succ_next')

    def __init__(self, order, n_vocab, eos, arrays, dropped=0, has_unk=False, tokens='symbols'):
        self.tokens = tokens
        self.order, self.n_vocab, self.eos, self.dropped, self.has_unk = int(order), int(n_vocab), int(eos), int(dropped), bool(has_unk)
        for name in self.ARRAYS:
            want = np.float32 if name in ('uni_logp', 'bo', 'succ_logp') else np.int32
            setattr(self, name, np.ascontiguousarray(arrays[name], want))
        self.n_nodes, self.n_succ = int(self.bo.shape[0]), int(self.succ_label.shape[0])
        if not (1 <= self.order <= MAX_ORDER and self.n_vocab >= 1 and 0 <= self.eos < self.n_vocab and self.n_nodes >= 1):
            raise ValueError('n-gram tables: bad order / label count / eos (%d, %d, %d)' % (self.order, self.n_vocab, self.eos))
        if not (self.uni_logp.shape == self.uni_next.shape == (self.n_vocab,) and self.bo_node.shape == (self.n_nodes,)
                and self.succ_off.shape == (self.n_nodes + 1,) and self.succ_logp.shape == self.succ_next.shape == (self.n_succ,)):
            raise ValueError('n-gram tables: the arrays do not fit together')
        self._dev = {}

    # ---- construction ------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_arpa(cls, path, char_list, tokens='symbols'):
        """The tables of the ARPA file ``path`` over the labels of ``char_list`` (the last one is eos)."""
        if tokens not in ('symbols', 'ids'):
            raise ValueError("tokens is 'symbols' or 'ids', not %r" % (tokens,))
        V = len(char_list)
        eos = V - 1
        grams_tok = read_arpa(path)
        sym = {c: i for i, c in enumerate(char_list)}
        unk = sym['<unk>'] if tokens == 'symbols' and '<unk>' in sym else V       # V: <unk> is no label itself, only what labels fall back to

        def label(tok):
            """(label or None, role): role 's' / 'e' for the sentence marks that share the label eos."""
            if tokens == 'symbols':
                if tok == '<s>':
                    return eos, 's'
                if tok == '</s>':
                    return eos, 'e'
                if tok == '<unk>':
                    return unk, ''
                return sym.get(tok), ''
            if tok == '<unk>':
                return unk, ''
            if tok.isdigit() and int(tok) < V:
                return int(tok), ''
            return None, ''

        vocab = {w[0]: label(w[0]) for w in grams_tok[0]}
        dropped = sum(1 for lab, _ in vocab.values() if lab is None)
        grams = []
        for k, level in enumerate(grams_tok, 1):
            out = {}
            for words, (logp, bo) in level.items():
                labs = [vocab.get(w, (None, '')) for w in words]
                if any(lab is None for lab, _ in labs):
                    continue
                g = tuple(lab for lab, _ in labs)
                role = labs[-1][1]
                old = out.get(g)
                if old is None:
                    out[g] = [None if role == 's' else logp * LN10, None if role == 'e' else bo * LN10]
                elif role == 's' and old[1] is None:
                    old[1] = bo * LN10                       # <s> gives the context [.. eos] its back-off
                elif role == 'e' and old[0] is None:
                    old[0] = logp * LN10                     # </s> gives the label eos its log-probability
                else:
                    raise ArpaError(0, 'the n-grams %r and another one are the same label sequence %r' % (' '.join(words), g))
            grams.append({g: (LOGZERO if v[0] is None else v[0], 0.0 if v[1] is None else v[1]) for g, v in out.items()})
        tables = cls.from_grams(grams, V, eos, unk=unk, dropped=dropped)
        tables.tokens = tokens
        return tables

    @classmethod
    def from_grams(cls, grams, n_vocab, eos, unk=None, dropped=0):
        """From ``grams[k-1] = {(l1, .., lk): (ln p, ln back-off)}`` over label ids, prefix-closed (the dictionary form).  ``unk``: the id that
        stands for the model's <unk> -- a label, or ``n_vocab`` for one that is no label itself; labels without a unigram score as it does."""
        V, order = int(n_vocab), len(grams)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError('orders 1 .. %d are supported, got %d' % (MAX_ORDER, order))
        unk = V if unk is None else int(unk)
        has_unk = (unk,) in grams[0]
        missing = [v for v in range(V) if (v,) not in grams[0]]
        # the labels an entry for <unk> stands for: itself when it is a label, and every label without a unigram
        unk_labels = sorted(set(([unk] if unk < V else []) + missing)) if has_unk else []
        node_of = {}
        for k in range(1, order):
            for g in sorted(grams[k - 1]):
                node_of[g] = len(node_of) + 1
        N = len(node_of) + 1
        bo, bo_node = np.zeros(N, np.float32), np.zeros(N, np.int32)
        for k in range(1, order):
            for g, (_, b) in grams[k - 1].items():
                nd = node_of[g]
                bo[nd] = np.float32(b)
                bo_node[nd] = _suffix_node(node_of, g[1:], order - 1)
        uni_logp, uni_next = np.full(V, np.float32(LOGZERO), np.float32), np.zeros(V, np.int32)
        for v in range(V):
            g = (v,) if (v,) in grams[0] else ((unk,) if has_unk else None)
            if g is not None:
                uni_logp[v] = np.float32(grams[0][g][0])
                uni_next[v] = node_of.get(g, 0)
        s_node, s_label, s_logp, s_next = [], [], [], []
        for k in range(2, order + 1):
            for g, (lp, _) in grams[k - 1].items():
                ctx = node_of.get(g[:-1])
                if ctx is None:
                    raise ValueError('n-gram %r: its prefix is not an n-gram' % (g,))
                nxt = node_of[g] if k < order else _suffix_node(node_of, g[1:], order - 1)
                last = g[-1]
                for lab in (unk_labels if last == unk and has_unk else ([last] if last < V else [])):
                    s_node.append(ctx), s_label.append(lab), s_logp.append(lp), s_next.append(nxt)
        s_node, s_label = np.asarray(s_node, np.int64), np.asarray(s_label, np.int64)
        at = np.lexsort((s_label, s_node))
        succ_off = np.zeros(N + 1, np.int64)
        np.add.at(succ_off, s_node + 1, 1)
        arrays = dict(uni_logp=uni_logp, uni_next=uni_next, bo=bo, bo_node=bo_node, succ_off=np.cumsum(succ_off), succ_label=s_label[at],
                      succ_logp=np.asarray(s_logp, np.float64)[at].astype(np.float32), succ_next=np.asarray(s_next, np.int64)[at])
        return cls(order, V, eos, arrays, dropped=dropped, has_unk=has_unk)

    # ---- persistence -------------------------------------------------------------------------------------------------------------------------
    def save(self, path):
        """The arrays and their scalars as .npz at exactly ``path``."""
        with open(path, 'wb') as f:
            np.savez(f, meta=np.asarray([self.order, self.n_vocab, self.eos, self.dropped, int(self.has_unk), int(self.tokens == 'ids')], np.int64),
                     **{name: getattr(self, name) for name in self.ARRAYS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            meta = [int(v) for v in z['meta']]
            return cls(meta[0], meta[1], meta[2], {name: z[name] for name in cls.ARRAYS}, dropped=meta[3], has_unk=bool(meta[4]),
                       tokens='ids' if meta[5] else 'symbols')

    # ---- the host arbiter --------------------------------------------------------------------------------------------------------------------
    def _chain(self, d):
        """The back-off chain d, bo_node[d], .. root of node d and, per level, the fp32 sum of the back-offs above it (deep end first)."""
        nodes, pre, acc = [], [], np.float32(0.0)
        for _ in range(MAX_ORDER):
            nodes.append(d), pre.append(acc)
            if d == 0:
                return nodes, pre
            acc = np.float32(acc + self.bo[d])
            d = int(self.bo_node[d])
        raise ValueError('a back-off chain of more than %d nodes' % MAX_ORDER)

    def advance(self, s, x):
        """The node after label ``x`` in node ``s``: along the chain of ``s`` the first node that has ``x`` among its successors."""
        for nd in self._chain(int(s))[0]:
            if nd == 0:
                return int(self.uni_next[x])
            a, b = int(self.succ_off[nd]), int(self.succ_off[nd + 1])
            e = a + int(np.searchsorted(self.succ_label[a:b], x))
            if e < b and self.succ_label[e] == x:
                return int(self.succ_next[e])

    def step_host(self, state, x):
        """re2e_ngram_step on the host, over the same fp32 arrays with numpy fp32 additions in the same order: ``state`` (n,) node ids or None
        (the root), ``x`` (n,) labels -> (state' (n,) int32, lp (n, V) fp32).  A state or a label out of range: NaN scores and state -1."""
        x = np.asarray(x, np.int64).reshape(-1)
        n, V = x.shape[0], self.n_vocab
        state = np.zeros(n, np.int64) if state is None else np.asarray(state, np.int64).reshape(-1)
        new, lp = np.full(n, -1, np.int32), np.full((n, V), np.nan, np.float32)
        for r in range(n):
            if not (0 <= state[r] < self.n_nodes and 0 <= x[r] < V):
                continue
            d = self.advance(state[r], int(x[r]))
            nodes, pre = self._chain(d)
            row = pre[-1] + self.uni_logp                          # fp32 + fp32 array: one rounding per element
            for nd, p in zip(nodes[-2::-1], pre[-2::-1]):          # shallow to deep: the deeper level wins
                a, b = int(self.succ_off[nd]), int(self.succ_off[nd + 1])
                row[self.succ_label[a:b]] = p + self.succ_logp[a:b]
            new[r], lp[r] = d, row
        return new, lp

    def score_host(self, seq, append_eos=True):
        """The fp32 terms re2e_ngram_score_seqs adds for one label sequence, from the context [eos] (a list of np.float32)."""
        node, terms = int(self.uni_next[self.eos]), []
        for x in list(seq) + ([self.eos] if append_eos else []):
            nodes, pre = self._chain(node)
            for nd, p in zip(nodes, pre):
                if nd == 0:
                    terms.append(np.float32(p + self.uni_logp[x]))
                    node = int(self.uni_next[x])
                    break
                a, b = int(self.succ_off[nd]), int(self.succ_off[nd + 1])
                e = a + int(np.searchsorted(self.succ_label[a:b], x))
                if e < b and self.succ_label[e] == x:
                    terms.append(np.float32(p + self.succ_logp[e]))
                    node = int(self.succ_next[e])
                    break
        return terms

    # ---- the device side ---------------------------------------------------------------------------------------------------------------------
    def tensors(self):
        """name -> torch tensor of every array (an empty successor list is one padding entry, so that every array has an address)."""
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)
        return {name: torch.from_numpy(pad(getattr(self, name)).copy()) for name in self.ARRAYS}

    def table_args(self, t):
        """The leading arguments of both entry points from the tensors ``t`` (name -> device tensor)."""
        return tuple(t[name].data_ptr() for name in self.ARRAYS) + (self.n_nodes, self.n_succ, self.n_vocab, self.order)

    def score_seqs(self, seqs, device, append_eos=True):
        """re2e_ngram_score_seqs: the summed natural-log probability of every label sequence of ``seqs`` in one launch (numpy float64)."""
        S = len(seqs)
        if S == 0:
            return np.zeros(0, np.float64)
        key = str(device)
        if key not in self._dev:
            self._dev[key] = {k: v.to(device) for k, v in self.tensors().items()}
        Lmax = max(1, max(len(s) for s in seqs))
        labels = np.zeros((S, Lmax), np.int32)
        for i, s in enumerate(seqs):
            labels[i, :len(s)] = np.asarray(s, np.int32)
        lab_d = torch.from_numpy(labels).to(device)
        len_d = torch.from_numpy(np.asarray([len(s) for s in seqs], np.int32)).to(device)
        out = _empty(S, dtype=torch.float64, device=device)
        with torch.cuda.device(device):
            call('re2e_ngram_score_seqs', *self.table_args(self._dev[key]), lab_d.data_ptr(), Lmax, len_d.data_ptr(), S, self.eos,
                 int(bool(append_eos)), out.data_ptr())
        return out.cpu().numpy()


def _empty(*shape, **kw):
    """Every output buffer of a step comes from here (tests hand out NaN-filled ones: a kernel must write all of it)."""
    return torch.empty(*shape, **kw)


class NgramLM(torch.nn.Module):
    """The predictor of a ClassifierWithState over ``NgramTables``: the arrays are buffers (``.to(device)`` moves them), the state is
    ``{'node': (n,) int32}`` -- dimension 0 is the row, so the searches' ``index_select(0, parents)`` carries it."""
    normalized = True            # forward returns log-probabilities (ClassifierWithState.predict_combined)
    logzero = LOGZERO

    def __init__(self, tables):
        super(NgramLM, self).__init__()
        if not isinstance(tables, NgramTables):
            raise TypeError('NgramLM takes NgramTables, got %s' % type(tables).__name__)
        self.tables = tables
        self.n_vocab, self.order = tables.n_vocab, tables.order
        for name, t in tables.tensors().items():
            self.register_buffer(name, t)

    @property
    def device(self):
        return self.uni_logp.device

    def forward(self, state, x):
        """``x``: the n last labels; ``state``: None (every row at the root) or {'node': (n,)} -> (state, log-probabilities (n, V))."""
        state, lp, _ = self.forward_combined(state, x)
        return state, lp

    def forward_combined(self, state, x, att=None, lm_weight=0.0):
        """``forward`` plus ``att + lm_weight * lp`` (product, then sum, each rounded to fp32) when ``att`` (n, V) is given, else None."""
        if self.training:
            raise Re2eError('NgramLM runs in evaluation mode only (call .eval())')
        dev = self.device
        if dev.type != 'cuda':
            raise Re2eError('the NgramLM is on %s: there is no CPU path (call .cuda())' % dev)
        if isinstance(x, torch.Tensor) and x.is_cuda:
            ids = x.to(device=dev, dtype=torch.int32).contiguous().view(-1)
        else:
            ids = host_to_dev(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, np.int32).reshape(-1), dev)
        n, V = ids.numel(), self.n_vocab
        if n < 1:
            raise Re2eError('NgramLM.forward needs at least one label')
        node = None
        if state is not None:
            if 'node' not in state or tuple(state['node'].shape) != (n,):
                raise Re2eError('NgramLM state: node is %s, expected (%d,): one row per label in x'
                                % (tuple(state['node'].shape) if 'node' in state else None, n))
            node = state['node'].to(device=dev, dtype=torch.int32).contiguous()
        w = float(np.float32(lm_weight))
        if att is not None:
            if tuple(att.shape) != (n, V) or att.dtype != torch.float32 or att.device != dev:
                raise Re2eError('NgramLM: att is %s %s on %s, expected (%d, %d) float32 on %s' % (tuple(att.shape), att.dtype, att.device, n, V, dev))
            att = att.contiguous()
        with torch.no_grad():
            if HOST_PATH:
                new, lp = self.tables.step_host(None if node is None else node.cpu().numpy(), ids.cpu().numpy())
                new, lp = torch.from_numpy(new).to(dev), torch.from_numpy(lp).to(dev)
                return {'node': new}, lp, (att + w * lp if att is not None else None)
            new, lp = _empty(n, dtype=torch.int32, device=dev), _empty(n, V, device=dev)
            comb = _empty(n, V, device=dev) if att is not None else None
            t = {name: getattr(self, name) for name in NgramTables.ARRAYS}
            call('re2e_ngram_step', *self.tables.table_args(t), node.data_ptr() if node is not None else None, ids.data_ptr(), n,
                 att.data_ptr() if att is not None else None, w, new.data_ptr(), lp.data_ptr(), comb.data_ptr() if comb is not None else None)
            return {'node': new}, lp, comb


def load_tables(path, char_list, tokens='symbols'):
    """The tables of the ARPA file ``path``: from ``path + '.npz'`` when that is newer than the file and fits the dictionary, else from the
    text, writing the cache (best effort: a read-only directory only costs the parse next time).  A binary KenLM file is refused."""
    if not path or not os.path.isfile(path):
        raise FileNotFoundError('no n-gram language model found at %s' % path)
    with open(path, 'rb') as f:
        head = f.read(64)
    if path.endswith('.bin') or head.startswith(b'mmap lm') or b'\x00' in head:
        raise Re2eError('%s is a binary KenLM file: only the ARPA text format is read; export ARPA (the file lmplz writes, before build_binary)' % path)
    cache = path + '.npz'
    if os.path.isfile(cache) and os.path.getmtime(cache) >= os.path.getmtime(path):
        try:
            tables = NgramTables.load(cache)
            if tables.n_vocab == len(char_list) and tables.tokens == tokens:
                return tables
        except Exception:
            pass                                                # a damaged cache: parse again
    tables = NgramTables.from_arpa(path, char_list, tokens)
    try:
        tables.save(cache)
    except OSError:
        pass
    return tables
