"""Float64 references of the decode-time kernels -- the CTC prefix scorers of csrc/ctc.hip (re2e_ctc_prefix_score, _batch, _cands) and the
few-row language-model kernels of csrc/rnnlm.hip (re2e_lm_lstm_cell, re2e_lm_output, re2e_lm_log_softmax_combine, re2e_lm_add_cands) -- and
the case tables of tests/test_dec_kernels_gpu.py.

Plain numpy / torch on the CPU, nothing imported from the product or from ``oracle``.  Every reference takes ``dtype``: float64 is the
yardstick, the SAME code in float32 says how far fp32 arithmetic alone is from it on a given input (``margin_ok``).  Pinned by
tests/test_refs64_dec_cpu.py: the prefix recursion to an enumeration of all V^T alignments and to the host scorer that follows upstream, the
LM references to torch's own modules on doubles.

Prefix scores (Watanabe et al., "Hybrid CTC/attention architecture for end-to-end speech recognition", Algorithm 2).  For a hypothesis g of
n labels, frame posteriors lpz (T, V) in the log domain and the forward variables r_prev (T, 2) of g (r[t][0] / r[t][1]: log-probability of
all alignments of frames 0 .. t to g that end in g's last label / in blank), a candidate label c gives

    start  = min(max(n, 1), T)                                          (the clamp: a hypothesis longer than the T frames)
    r[start-1] = (lpz[0][c], LOGZERO) if n == 0 else (LOGZERO, LOGZERO)
    phi[t] = r_prev[t][1] if n > 0 and c == g[-1] else logaddexp(r_prev[t][0], r_prev[t][1])
    r[t][0] = logaddexp(r[t-1][0], phi[t-1]) + lpz[t][c];   r[t][1] = logaddexp(r[t-1][0], r[t-1][1]) + lpz[t][blank]      start <= t < T
    log_psi = logaddexp over t of (phi[t-1] + lpz[t][c]), seeded with r[start-1][0];   c == <eos>: log_psi = logaddexp(r_prev[T-1])

with LOGZERO = -1e10 standing for log 0.  Rows t < start - 1 of r are never read by the next position (upstream leaves them unset), so they
are exempt from every comparison; a value <= -1e9 is "dead" (LOGZERO plus whatever was added to it): a kernel must be dead exactly where
float64 is, and live values are compared relative to the largest LIVE magnitude -- relative to the tensor's max every comparison would be
blind beside 1e10.

``PREFIX_CASES``: one row per thing a kernel can get wrong, at the smallest shape that reaches it (the kernels stage 256 entries per
trip: 2T > 256, T > 256, V > 256; ctc_beam 1, 64 and V; T = 1 and 2; hypotheses as long as and longer than the utterance; attention rows the
top-k cannot rank in the ordinary way; more than 64 KB of dynamic LDS, V + 3T floats; candidate lists of 1, 255, 256, 257 labels, proper
subsets, duplicates; several utterances of different lengths in one launch).  Every row is chained over four output positions
(``prefix_chain``); the inputs of every position are fp32 tensors (the float64 chain's results, rounded), so the kernel, the fp32 run and
the float64 run of a position read the same numbers.

``LM_CELL_CASES`` / ``LM_OUT_CASES`` carry the kernel form each row must reach (what re2e_lm_plan has to answer for it):
lm_cell_kernel<R, VI, VH> with R in 4 / 8 / 16 by the row count and (VI, VH) in (4,4), (4,2), (2,2), (1,1) by the widths and by the
alignment of the operands; lm_out_kernel<R, VEC>.  ``LSM_CASES``: re2e_lm_log_softmax_combine on both sides of 1024 (one lane pass), of 8192
(the logits a workgroup keeps in registers) and at one more full pass of its tail loop.
"""
import functools

import numpy as np
import torch

from refs64 import margin_ok, rel_err, rnd, BAR_GRAD          # noqa: F401  (re-exported)
from refs64_fsrnn import BAR_OUT                                  # noqa: F401  h and c of the few-row cell, of the tensor's max

LOGZERO = -1e10
DEAD = -1e9
BAR_PREFIX = 2e-5          # prefix scores, local scores and live forward variables, of the live max (the project's bar for them, test_kernels_gpu.py)
BAR_LOGITS = 2e-4          # logits of the output layer, of the tensor's max (test_recog_lm_gpu.py: test_few_row_kernels_at_production_widths)
ATT_WEIGHT, CTC_WEIGHT = float(np.float32(0.7)), float(np.float32(0.3))


def _np(dtype):
    return {torch.float64: np.float64, torch.float32: np.float32}[dtype]


# ---------------------------------------------------------------------------------------------
# prefix scores
# ---------------------------------------------------------------------------------------------
def prefix_initial_state(lpz, blank, dtype=torch.float64):
    """Forward variables of the empty hypothesis: r[t] = (LOGZERO, sum of lpz[0 .. t][blank]) -> (T, 2)."""
    f = _np(dtype)
    x = np.asarray(lpz).astype(f)
    r = np.full((x.shape[0], 2), LOGZERO, dtype=f)
    r[:, 1] = np.cumsum(x[:, blank], dtype=f)
    return r


def prefix_rows(lpz, ns, lasts, cands, r_prev, blank, eos, dtype=torch.float64):
    """Algorithm 2 for several hypotheses of one utterance at once.  lpz (T,V); ns, lasts (nh): length and last label of each hypothesis;
    cands (nh,nc) labels; r_prev (nh,T,2) -> (log_psi (nh,nc), r_new (nh,nc,T,2)) as numpy arrays of ``dtype``.  Rows t < start - 1 of
    r_new hold LOGZERO."""
    f = _np(dtype)
    x = np.asarray(lpz).astype(f)
    T = x.shape[0]
    ns, lasts, cands = np.asarray(ns).reshape(-1), np.asarray(lasts).reshape(-1), np.asarray(cands)
    rp = np.asarray(r_prev).astype(f)
    nh, nc = cands.shape
    start = np.minimum(np.maximum(ns, 1), T)[:, None]                                  # (nh,1)
    r_sum = np.logaddexp(rp[:, :, 0], rp[:, :, 1])                                     # (nh,T)
    rep = (ns[:, None] > 0) & (cands == lasts[:, None])                                # (nh,nc)
    zero = f(LOGZERO)
    cur_n = np.where(ns[:, None] == 0, x[0][cands], zero).astype(f)                    # r[start-1]
    cur_b = np.full((nh, nc), zero, dtype=f)
    r = np.full((nh, nc, T, 2), zero, dtype=f)
    log_psi = cur_n.copy()
    at = np.broadcast_to(start - 1 == 0, (nh, nc))
    r[:, :, 0, 0], r[:, :, 0, 1] = np.where(at, cur_n, zero), np.where(at, cur_b, zero)
    xb = x[:, blank]
    for t in range(1, T):
        phi = np.where(rep, rp[:, t - 1, 1][:, None], r_sum[:, t - 1][:, None])
        xs = x[t][cands]
        nn = np.logaddexp(cur_n, phi) + xs
        nb = np.logaddexp(cur_n, cur_b) + xb[t]
        act = np.broadcast_to(t >= start, (nh, nc))
        log_psi = np.where(act, np.logaddexp(log_psi, phi + xs), log_psi)
        cur_n, cur_b = np.where(act, nn, cur_n), np.where(act, nb, cur_b)
        keep = np.broadcast_to(t >= start - 1, (nh, nc))                               # (t == start - 1: the seed itself)
        r[:, :, t, 0], r[:, :, t, 1] = np.where(keep, cur_n, zero), np.where(keep, cur_b, zero)
    log_psi = np.where(cands == eos, r_sum[:, T - 1][:, None], log_psi)
    return log_psi.astype(f), r


def prefix_ref(lpz, y, cs, r_prev, blank, eos, dtype=torch.float64):
    """One hypothesis: y = [<sos>, labels ...] (n = len(y) - 1), candidates cs, r_prev (T,2) -> (log_psi (len(cs),), r_new (len(cs),T,2))."""
    psi, r = prefix_rows(lpz, [len(y) - 1], [y[-1]], np.asarray(cs).reshape(1, -1), np.asarray(r_prev)[None], blank, eos, dtype)
    return psi[0], r[0]


def prefix_brute(lpz, g, blank):
    """By enumeration of all V^T frame labellings (float64, probabilities): for the label sequence g (no <sos>) -> (log prefix probability
    of g = log P(the collapsed labelling STARTS with g), r (T,2) with r[t][0] / r[t][1] = log P(frames 0 .. t collapse to exactly g and frame
    t carries g's last label / blank)).  log 0 is -inf here."""
    import itertools
    p = np.exp(np.asarray(lpz, dtype=np.float64))
    T, V = p.shape
    g = list(g)

    def collapse(path):
        out, prev = [], None
        for s in path:
            if s != prev and s != blank:
                out.append(s)
            prev = s
        return out

    prefix = 0.0
    r = np.zeros((T, 2))
    for path in itertools.product(range(V), repeat=T):
        pr = 1.0
        for t, s in enumerate(path):
            pr *= p[t, s]
        if collapse(path)[:len(g)] == g:
            prefix += pr
    for t in range(T):
        for path in itertools.product(range(V), repeat=t + 1):
            if collapse(path) == g:
                pr = 1.0
                for u, s in enumerate(path):
                    pr *= p[u, s]
                r[t, 1 if path[-1] == blank else 0] += pr
    with np.errstate(divide='ignore'):
        return np.log(prefix), np.log(r)


def classes(a):
    """0 live, 1 dead (finite, <= -1e9), 2 -inf, 3 NaN / +inf: a kernel must agree with float64 on the class of every element."""
    a = np.asarray(a, dtype=np.float64)
    c = np.zeros(a.shape, dtype=np.int8)
    c[np.isfinite(a) & (a <= DEAD)] = 1
    c[np.isneginf(a)] = 2
    c[np.isnan(a) | np.isposinf(a)] = 3
    return c


def live_err(got, ref, mask=None):
    """max |got - ref| over the LIVE entries of ref (inside ``mask``), relative to the largest live |ref| of the WHOLE tensor; 0 when
    nothing is live.  The classes have to agree first (``classes``)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    live = classes(ref) == 0
    if not live.any():
        return 0.0
    scale = np.abs(ref[live]).max()
    if mask is not None:
        live = live & mask
        if not live.any():
            return 0.0
    err = np.abs(got[live] - ref[live]).max()
    if not np.isfinite(err):
        return float('inf')
    return float(err / scale) if scale > 0 else (0.0 if err == 0 else 1.0)


def read_mask(shape, starts):
    """(nh,nc,T,2) mask of the state rows the next position reads: t >= start - 1 of each hypothesis."""
    nh, nc, T, _ = shape
    t = np.arange(T)[None, None, :, None]
    return np.broadcast_to(t >= (np.asarray(starts).reshape(nh, 1, 1, 1) - 1), shape)


def topk_labels(att_row, k):
    """What the top-k entry points must choose: the first k labels of a stable descending sort of the fp32 row, NaN ranked as -inf."""
    a = np.asarray(att_row, dtype=np.float32)
    a = np.where(np.isnan(a), -np.inf, a)
    return np.argsort(-a, kind='stable')[:k]


# name, entry points, T (a list: the utterances of a _batch launch), V, ctc_beam (top-k) or the candidate list's kind, options
#   peak: peaked posteriors; deep: the last position also carries hypotheses of T and T + 3 labels; weak: degenerate attention rows
#   bar (scores), bar_r (states): set where the fp32 CPU run of the reference is not within a quarter of BAR_PREFIX -- 4 x that run's
#   distance, one digit, rounded up
def _row(name, entries, T, V, cb=None, cands=None, bar=BAR_PREFIX, bar_r=BAR_PREFIX, **opt):
    return dict(name=name, entries=entries, T=T, V=V, cb=cb, cands=cands, bar=bar, bar_r=bar_r, opt=opt)


PREFIX_CASES = [
    _row('one-trip', ('topk', 'cands'), 57, 23, cb=7, cands=('sorted', 23)),
    _row('2T-over-256', ('topk', 'cands'), 129, 40, cb=7, cands=('subset', 9)),
    _row('T-over-256', ('topk', 'cands'), 257, 40, cb=7, cands=('dups', 12)),
    _row('V-over-256-cb64', ('topk',), 30, 300, cb=64),
    _row('cb1', ('topk',), 20, 11, cb=1),
    _row('cb-is-V', ('topk',), 20, 5, cb=5),
    _row('T1', ('topk', 'cands'), 1, 9, cb=4, cands=('subset', 5)),
    _row('T2', ('topk', 'cands'), 2, 9, cb=4, cands=('subset', 5)),
    _row('deep', ('topk', 'cands'), 3, 9, cb=4, cands=('subset', 5), deep=True),
    _row('weak-rows', ('topk',), 12, 13, cb=5, weak=True),
    # fp32 on the CPU (numpy), of the live max: scores 3e-8, local scores 1.3e-7: within the quarter.  States 6.2e-5: after thousands of frames
    # the forward variables stand near -1.8e4, where an fp32 ulp is 1e-3 and the log1p term of most logaddexp calls is below half of it, so
    # it is dropped frame after frame, in one direction.  The states' bar of this row is therefore 4 x 6.2e-5 -> 3e-4.
    _row('lds-over-64k', ('topk',), 5400, 300, cb=15, peak=True, bar_r=3e-4),
    _row('ncand1', ('cands',), 30, 300, cands=('subset', 1)),
    _row('ncand255', ('cands',), 30, 300, cands=('subset', 255)),
    _row('ncand256', ('cands',), 30, 300, cands=('subset', 256)),
    _row('ncand257', ('cands',), 30, 300, cands=('subset', 257)),
    _row('all-V300-sorted', ('cands',), 41, 300, cands=('sorted', 300)),
    _row('batch', ('batch',), [37, 1, 23], 12, cb=6),
    _row('batch-2T-over-256', ('batch',), [131, 1, 77], 40, cb=15),
    _row('batch-weak-deep', ('batch',), [5, 1, 3], 13, cb=5, weak=True, deep=True),
]
PREFIX_IDS = [c['name'] for c in PREFIX_CASES]
POSITIONS = 4
BLANK = 0


def _posteriors(g, T, V, peak):
    x = 2.0 * rnd(g, T, V)
    if peak:                           # as a trained model's: one label, mostly blank, stands out in every frame
        lab = torch.randint(1, V, (T,), generator=g)
        lab[torch.rand(T, generator=g) < 0.8] = BLANK
        x[torch.arange(T), lab] += 6.0
    return torch.log_softmax(x, 1).numpy()


@functools.lru_cache(maxsize=None)
def prefix_chain(name, entry):
    """The launches of a row on one entry point: a list of POSITIONS dicts with the fp32 inputs of the position (lpz (U,Tmax,V), tlen, utt, att
    (nh,V), r_prev (nh,Tmax,2), last, olen, prev), the candidate labels it must score (``cands`` (nh,nc): for the top-k entry points what
    they must choose themselves), and the float64 / float32 results (psi, local (nh,nc), r (nh,nc,Tmax,2); entries at t >= T_u are LOGZERO),
    ``starts`` (nh).  Hypotheses of the next position: survivors of this one -- the repeated label, <eos> and blank among them wherever
    they were candidates -- beside the empty hypothesis and one of a single label, so that a launch mixes out_len 0, 1 and >= 2."""
    case = PREFIX_CASES[PREFIX_IDS.index(name)]
    assert entry in case['entries']
    Ts = case['T'] if isinstance(case['T'], list) else [case['T']]
    U, Tmax, V, opt = len(Ts), max(Ts), case['V'], case['opt']
    eos = V - 1
    g = torch.Generator().manual_seed(9000 + 7 * PREFIX_IDS.index(name) + ('topk', 'cands', 'batch').index(entry))
    lpz = np.zeros((U, Tmax, V), dtype=np.float32)
    for u, T in enumerate(Ts):
        lpz[u, :T] = _posteriors(g, T, V, opt.get('peak', False))
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)

    def root(u):
        st = np.full((Tmax, 2), 123.0, dtype=np.float32)                        # beyond T_u: a finite decoy, never to be read
        st[:Ts[u]] = f32(prefix_initial_state(lpz[u, :Ts[u]], BLANK))
        return dict(u=u, y=[eos], state=st, score=np.float32(0.0))

    hyps = [root(u) for u in range(U)]
    hyps = [hyps[i] for i in sorted(range(U), key=lambda i: -i)]                # utterances in descending order first: rows interleave below
    launches = []
    for pos in range(POSITIONS):
        if opt.get('deep') and pos == POSITIONS - 1:
            extra = []
            for hp in hyps[:2]:
                for n in (Ts[hp['u']], Ts[hp['u']] + 3):
                    lab = [int(v) for v in torch.randint(1, V - 1, (n,), generator=g)]
                    extra.append(dict(u=hp['u'], y=[eos] + lab, state=hp['state'], score=np.float32(-5.0)))
            hyps = hyps + extra
        nh = len(hyps)
        ns = np.array([len(hp['y']) - 1 for hp in hyps])
        lasts = np.array([hp['y'][-1] for hp in hyps])
        att = torch.log_softmax(rnd(g, nh, V), 1).numpy()
        if V > 9:
            att[:, 5] = att[:, 9]                                                # a tie: the lower label first
        for k in range(nh):
            if ns[k] > 0 and (k + pos) % 2 == 1:
                att[k, lasts[k]] = 0.6                                           # the repeated label is a candidate
        att[pos % nh, eos] = 0.9
        att[(pos + 1) % nh, BLANK] = 0.7
        if opt.get('weak') and pos >= 1:
            att[0, :] = -np.inf                                                  # fewer than ctc_beam finite scores
            att[0, 7], att[0, 3] = -0.5, -1.0
            if nh > 1:
                att[1, 4] = np.nan                                               # a NaN among finite scores
        if entry == 'cands':
            kind, nc = case['cands']
            if kind == 'sorted':
                cands = np.stack([topk_labels(att[k], nc) for k in range(nh)])
            else:
                rows = []
                for k in range(nh):
                    head = [int(lasts[k]) if ns[k] > 0 else eos, eos, BLANK][(k + pos) % 3:]
                    head = list(dict.fromkeys(head))
                    rest = [int(v) for v in torch.randperm(V, generator=g) if int(v) not in head]
                    lst = (head + rest)[:nc]
                    if kind == 'dups':
                        lst[len(lst) // 2:] = lst[:len(lst) - len(lst) // 2]      # the second half repeats the first
                    rows.append(lst)
                cands = np.array(rows)
        else:
            cands = np.stack([topk_labels(att[k], case['cb']) for k in range(nh)])
        nc = cands.shape[1]
        r_prev = np.stack([hp['state'] for hp in hyps])
        prev = np.array([hp['score'] for hp in hyps], dtype=np.float32)
        utt = np.array([hp['u'] for hp in hyps])
        att_c = np.take_along_axis(np.where(np.isnan(att), -np.inf, att) if entry != 'cands' else att, cands, 1)
        res = {}
        for dtype in (torch.float64, torch.float32):
            f = _np(dtype)
            psi, r = np.full((nh, nc), np.nan, dtype=f), np.full((nh, nc, Tmax, 2), f(LOGZERO), dtype=f)
            for u, T in enumerate(Ts):
                rows = np.nonzero(utt == u)[0]
                if len(rows):
                    psi[rows], r[rows, :, :T] = prefix_rows(lpz[u, :T], ns[rows], lasts[rows], cands[rows], r_prev[rows, :T], BLANK, eos, dtype)
            with np.errstate(invalid='ignore'):
                local = f(ATT_WEIGHT) * att_c.astype(f) + f(CTC_WEIGHT) * (psi - prev[:, None].astype(f))
            res[dtype] = dict(psi=psi, local=local, r=r)
        r64 = res[torch.float64]
        launches.append(dict(T=Ts, Tmax=Tmax, V=V, U=U, eos=eos, lpz=lpz, tlen=np.array(Ts), utt=utt, att=att, r_prev=r_prev, last=lasts, olen=ns,
                             prev=prev, cands=cands, starts=np.minimum(np.maximum(ns, 1), np.array(Ts)[utt]), f64=r64, f32=res[torch.float32],
                             flags=dict(repeat=bool(((ns[:, None] > 0) & (cands == lasts[:, None])).any()), eos=bool((cands == eos).any()),
                                        blank=bool((cands == BLANK).any()), olens=sorted(set(np.minimum(ns, 2).tolist())))))
        # survivors (a dead score -- a hypothesis out of frames -- is not extended: its score would be LOGZERO, the next difference noise)
        nxt, seen = [], set()

        def take(k, j):
            if (k, j) in seen or classes(r64['psi'][k, j]) != 0 or len(nxt) >= 5:
                return
            seen.add((k, j))
            st = np.full((Tmax, 2), 123.0, dtype=np.float32)
            st[:Ts[utt[k]]] = f32(r64['r'][k, j, :Ts[utt[k]]])
            nxt.append(dict(u=int(utt[k]), y=hyps[k]['y'] + [int(cands[k, j])], state=st, score=f32(r64['psi'][k, j])))

        for k in range(nh):
            for j in range(nc):
                c = int(cands[k, j])
                if (ns[k] > 0 and c == lasts[k]) or c == eos or c == BLANK:
                    take(k, j)
        for k in range(nh):
            take(k, 0)
            take(k, nc // 2)
            take(k, nc - 1)
        keep = [hp for hp in hyps if len(hp['y']) - 1 == 0][:U] + [hp for hp in hyps if len(hp['y']) - 1 == 1][:1]
        hyps = [h for pair in zip(nxt, keep) for h in pair] + nxt[len(keep):] + keep[len(nxt):]       # interleaved: utterances and lengths mix
    return launches


# ---------------------------------------------------------------------------------------------
# the few-row LM kernels
# ---------------------------------------------------------------------------------------------
def cell_ref(x, w_ih, w_hh, b_ih, b_hh, h_prev, c_prev, dtype=torch.float64):
    """nn.LSTMCell (gate order i, f, g, o) for the rows of x (n,I); h_prev / c_prev None: zeros -> (h, c)."""
    cv = lambda t: t.detach().to(dtype)
    n, H = x.shape[0], w_hh.shape[1]
    hp = cv(h_prev) if h_prev is not None else torch.zeros(n, H, dtype=dtype)
    cp = cv(c_prev) if c_prev is not None else torch.zeros(n, H, dtype=dtype)
    pi, pf, pg, po = (cv(x) @ cv(w_ih).t() + cv(b_ih) + hp @ cv(w_hh).t() + cv(b_hh)).chunk(4, 1)
    c = torch.sigmoid(pf) * cp + torch.sigmoid(pi) * torch.tanh(pg)
    return torch.sigmoid(po) * torch.tanh(c), c


def out_ref(h, w, b, dtype=torch.float64):
    return h.detach().to(dtype) @ w.detach().to(dtype).t() + b.detach().to(dtype)


def lsm_ref(logits, dtype=torch.float64):
    x = logits.detach().to(dtype)
    m = x.max(1, keepdim=True).values
    return x - m - torch.log(torch.exp(x - m).sum(1, keepdim=True))


def comb_fp32(att, lm_weight, lsm):
    """att + fl(w * lsm) with the product and the sum rounded separately in fp32 (what the kernel documents), from fp32 tensors."""
    w = torch.tensor(lm_weight, dtype=torch.float32)
    return att.float() + (w * lsm.float())


def add_cands_fp32(local, lm, cand, lm_weight):
    """local[k][j] + fl(w * lm[k][cand[k][j]]) in fp32; a label outside [0, V) gives NaN."""
    V = lm.shape[1]
    ok = (cand >= 0) & (cand < V)
    gathered = torch.gather(lm.float(), 1, cand.clamp(0, V - 1).long())
    out = local.float() + torch.tensor(lm_weight, dtype=torch.float32) * gathered
    out[~ok] = float('nan')
    return out


LM_NS = (1, 4, 5, 8, 9, 16, 17, 33, 64)


def rows_per_trip(n):
    return 4 if n <= 4 else 8 if n <= 8 else 16


def _cell(name, n, I, H, form, x='dense', ldx=None, state='both', off=None):
    """x: 'dense' rows or 'ids' (a table of n + 3 rows gathered by ids); ldx: leading dimension of x (default I); state: 'both', 'none'
    (h_prev = c_prev = NULL), 'h' (c_prev alone NULL), 'c' (h_prev alone NULL); off: operand -> bytes past a 16-byte boundary."""
    return dict(name=name, n=n, I=I, H=H, x=x, ldx=ldx or I, state=state, off=off or {}, form=(rows_per_trip(n),) + form)


def _cell_cases():
    cs = []
    widths = (((8, 12), (4, 4)), ((8, 10), (4, 2)), ((6, 12), (2, 2)), ((6, 10), (2, 2)), ((5, 7), (1, 1)), ((4, 7), (1, 1)))
    states = ('both', 'both', 'none', 'h', 'both', 'c')
    for wi, ((I, H), form) in enumerate(widths):
        for ni, n in enumerate(LM_NS):
            k = wi + ni
            cs.append(_cell('I%d-H%d-n%d' % (I, H, n), n, I, H, form, x='ids' if k % 2 else 'dense', state=states[k % 6]))
    # operands 4 or 8 bytes off a 16-byte boundary at widths that would take 16-byte loads
    for op, by, form in (('x', 4, (1, 1)), ('w_ih', 8, (2, 2)), ('w_hh', 8, (4, 2)), ('h_prev', 4, (1, 1)), ('h_prev', 8, (4, 2)), ('w_hh', 4, (1, 1)),
                         ('x', 8, (2, 2))):
        cs.append(_cell('I8-H8-n5-%s+%d' % (op, by), 5, 8, 8, form, off={op: by}))
    # the contraction below one pass of the workgroup's 128 lanes, exactly one pass, one past it, per load width
    for K in (508, 512, 516):
        cs.append(_cell('K%d-vec4' % K, 5, K, K, (4, 4), x='ids' if K == 512 else 'dense'))
    for K, off in ((254, {}), (256, {'w_ih': 8, 'w_hh': 8}), (258, {})):
        cs.append(_cell('K%d-vec2' % K, 5, K, K, (2, 2), off=off))
    for K, off in ((127, {}), (128, {'w_ih': 4, 'w_hh': 4}), (129, {})):
        cs.append(_cell('K%d-vec1' % K, 5, K, K, (1, 1), off=off))
    # rows of x wider than I: 16-byte rows stay, odd rows demote VI (and with it the pair)
    cs.append(_cell('I8-H12-ldx12', 9, 8, 12, (4, 4), ldx=12))
    cs.append(_cell('I8-H12-ldx9', 9, 8, 12, (1, 1), ldx=9))
    cs.append(_cell('I8-H12-ids-ldx10', 5, 8, 12, (2, 2), x='ids', ldx=10))
    # the recipe's widths: layer 1 (embedding 256 -> 650, gathered) and layer 2 (650 -> 650, dense); H = 650: rows on 8-byte boundaries
    cs.append(_cell('recipe-l1', 12, 256, 650, (4, 2), x='ids'))
    cs.append(_cell('recipe-l2', 33, 650, 650, (2, 2)))
    cs.append(_cell('recipe-l1-first', 1, 256, 650, (4, 2), x='ids', state='none'))
    return cs


LM_CELL_CASES = _cell_cases()


def _out(name, n, V, H, vec, off=None):
    return dict(name=name, n=n, V=V, H=H, off=off or {}, form=(rows_per_trip(n), vec))


def _out_cases():
    cs = []
    k = 0
    for H, vec in ((12, 4), (10, 2), (7, 1)):
        for V in (1, 3, 4, 5):
            for n in (LM_NS[k % 9], LM_NS[(k + 4) % 9]):
                cs.append(_out('V%d-H%d-n%d' % (V, H, n), n, V, H, vec))
            k += 1
    for n in LM_NS:
        cs.append(_out('V5-H12-n%d-all-n' % n, n, 5, 12, 4))
    cs.append(_out('V5-H12-n5-h+8', 5, 5, 12, 2, off={'h': 8}))
    cs.append(_out('V5-H12-n5-w+4', 5, 5, 12, 1, off={'w': 4}))
    cs.append(_out('recipe-V4233-H650', 12, 4233, 650, 2))
    cs.append(_out('V4233-H652', 5, 4233, 652, 4))
    cs.append(_out('V4233-H650-n64', 64, 4233, 650, 2))
    return cs


LM_OUT_CASES = _out_cases()


def cell_inputs(row):
    """x / table ~ N(0,1), weights ~ N(0, 1/K) (every product as large as its addend), biases ~ 0.3 N(0,1), |h_prev| < 1, c_prev ~ 0.7 N(0,1)."""
    n, I, H, ldx = row['n'], row['I'], row['H'], row['ldx']
    g = torch.Generator().manual_seed(5000 + 1000 * n + 10 * I + H)
    nrow = n + 3 if row['x'] == 'ids' else n
    xfull = rnd(g, nrow, ldx)
    ids = torch.randint(0, nrow, (n,), generator=g).to(torch.int32) if row['x'] == 'ids' else None
    if ids is not None and n > 1:
        ids[n - 1] = ids[0]                                                       # a repeated id
    d = dict(xfull=xfull, ids=ids, w_ih=rnd(g, 4 * H, I, scale=I ** -0.5), w_hh=rnd(g, 4 * H, H, scale=H ** -0.5), b_ih=rnd(g, 4 * H, scale=0.3),
             b_hh=rnd(g, 4 * H, scale=0.3), h_prev=torch.tanh(rnd(g, n, H)) if row['state'] in ('both', 'h') else None,
             c_prev=rnd(g, n, H, scale=0.7) if row['state'] in ('both', 'c') else None)
    d['x'] = (xfull[ids.long()] if ids is not None else xfull)[:, :I]
    return d


def cell_case_ref(d, dtype=torch.float64):
    return cell_ref(d['x'], d['w_ih'], d['w_hh'], d['b_ih'], d['b_hh'], d['h_prev'], d['c_prev'], dtype)


def out_inputs(row):
    n, V, H = row['n'], row['V'], row['H']
    g = torch.Generator().manual_seed(6000 + 1000 * n + 10 * H + V)
    return dict(h=torch.tanh(rnd(g, n, H)), w=rnd(g, V, H, scale=H ** -0.5), b=rnd(g, V, scale=0.3))


LSM_CASES = [(V, n) for V in (1, 1023, 1024, 1025, 8191, 8192, 8193, 9217) for n in (1, 3)]


def lsm_inputs(V, n):
    """Row 0: logits spread over +-80 (the max subtraction); row 1: 2 N(0,1); row 2: all logits equal.  att ~ log_softmax."""
    g = torch.Generator().manual_seed(7000 + 10 * V + n)
    x = 2.0 * rnd(g, n, V)
    x[0] = rnd(g, V) + torch.where(torch.arange(V) % 2 == 0, 80.0, -80.0)
    if n > 2:
        x[2] = 1.25
    return dict(logits=x, att=torch.log_softmax(rnd(g, n, V), 1), lm_weight=0.3 if (V + n) % 2 else 0.0)
