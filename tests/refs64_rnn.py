"""Float64 reference of the bidirectional LSTM recurrence at its C-ABI contract (re2e_lstm_seq_fwd / re2e_lstm_seq_bwd, csrc/lstm.hip) and
the inputs of tests/test_recurrence_kernels_gpu.py.

Plain torch on the CPU, autograd for the backward, nothing imported from the product or from ``oracle``; pinned to a packed bidirectional
``nn.LSTM`` in double by tests/test_refs64_rnn_cpu.py.  Like the references of tests/refs64.py it takes ``dtype``: float64 is the yardstick,
the SAME code in float32 says how far fp32 arithmetic alone is from it on a given input (``margin_ok``).

``RNN_CASES`` holds one row per kernel form the launch plans (csrc/lstm.hip plan_fwd / plan_bwd) can name on a 256-CU chip under the
switches the library reads on every call; tests/test_refs64_rnn_cpu.py checks that the table is closed under those plans.
"""
import torch

from refs64 import margin_ok, rel_err, rnd          # noqa: F401  (re-exported: the tests of the recurrence use them through this module)

# the project's own bars (tests/test_kernels_gpu.py: test_bilstm)
BAR_RNN_OUT = 1e-4         # y, c and the activated gates, of the tensor's max
BAR_RNN_GRAD = 2e-4        # d(pre-activation gates) and dbias, of the tensor's max

QUANTITIES = (('y', BAR_RNN_OUT), ('c', BAR_RNN_OUT), ('gates_f', BAR_RNN_OUT), ('gates_r', BAR_RNN_OUT),
              ('dgates_f', BAR_RNN_GRAD), ('dgates_r', BAR_RNN_GRAD), ('dbias', BAR_RNN_GRAD))

# deliberate mistakes the sensitivity test applies to the reference (never used for a yardstick)
MISTAKES = {
    'a': 'input and forget gate swapped',
    'b': 'the reverse direction started at T - 1 instead of len_b - 1',
    'c': 'the last four hidden units left out of h W_hh^T',
    'd': 'dy of padded rows not masked',
    'e': 'the forward and reverse W_hh exchanged',
}


def valid_mask(lens, T):
    """(T,B) bool: frame t of utterance b exists."""
    return torch.arange(T).unsqueeze(1) < torch.as_tensor(lens).long().unsqueeze(0)


def _direction(x, whh, valid, reverse, mistake):
    """One direction over pre-activations x (T,B,4H) (finite everywhere) -> (h carried out of every step BEFORE the output mask (T,B,H),
    c (T,B,H) masked, activated gates (T,B,4H) masked).  Packed-sequence semantics: a frame t >= len_b leaves the state as it is, so the
    reverse direction, which walks t = T-1 .. 0, reaches t = len_b - 1 with the zero state it started from."""
    T, B, H4 = x.shape
    H = H4 // 4
    w = whh
    if mistake == 'c':
        w = torch.cat([whh[:, :H - 4], torch.zeros_like(whh[:, H - 4:])], 1)
    h, c = x.new_zeros(B, H), x.new_zeros(B, H)
    hs, cs, gs = [None] * T, [None] * T, [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        pre = x[t] + h @ w.t()
        pi, pf, pg, po = pre.chunk(4, 1)
        if mistake == 'a':
            pi, pf = pf, pi
        gi, gf, gg, go = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
        c_new = gf * c + gi * gg
        h_new = go * torch.tanh(c_new)
        m = valid[t].unsqueeze(1)
        keep = torch.ones_like(m) if (mistake == 'b' and reverse) else m
        c, h = torch.where(keep, c_new, c), torch.where(keep, h_new, h)
        hs[t] = h_new
        cs[t] = torch.where(m, c_new, torch.zeros_like(c_new))
        gs[t] = torch.where(m, torch.cat([gi, gf, gg, go], 1), torch.zeros_like(pre))
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def lstm_seq_forward(xg_f, xg_r, whh_f, whh_r, lens, mistake=None):
    """The differentiable core, in the dtype of its inputs: xg_* (T,B,4H) pre-activations x W_ih^T + b_ih + b_hh in gate order i, f, g, o,
    whh_* (4H,H) as nn.LSTM stores them, lens (B,) -> (y (T,B,2H) and c (T,B,2H): forward half | reverse half, zero beyond each length; the
    activated gates of each direction (T,B,4H), zero beyond the length; y before the output mask, which only mistake 'd' uses).
    The pre-activations of a frame t >= len_b are never read: they may hold NaN."""
    T = xg_f.shape[0]
    valid = valid_mask(lens, T)
    m3 = valid.unsqueeze(2)
    if mistake == 'e':
        whh_f, whh_r = whh_r, whh_f
    outs = []
    for x, w, reverse in ((xg_f, whh_f, False), (xg_r, whh_r, True)):
        if not (mistake == 'b' and reverse):        # (that mistake reads the padded frames: its caller leaves finite values there)
            x = torch.where(m3, x, torch.zeros_like(x))
        outs.append(_direction(x, w, valid, reverse, mistake))
    (hf, cf, gf), (hr, cr, gr) = outs
    raw = torch.cat([hf, hr], 2)
    y = torch.where(m3, raw, torch.zeros_like(raw))
    return y, torch.cat([cf, cr], 2), gf, gr, raw


def lstm_seq_ref(xg_f, xg_r, whh_f, whh_r, lens, dy, dtype=torch.float64, mistake=None):
    """What re2e_lstm_seq_fwd / _bwd produce, as a dict of detached tensors: y, c (T,B,2H) zero beyond each length; gates_f, gates_r (T,B,4H)
    activated, zero beyond the length; dgates_f, dgates_r (T,B,4H) = d sum(y * dy) / d pre-activations, zero beyond the length (``dy``
    (T,B,2H) carries values in the padded rows too: they must not leak); dbias (2,4H) = the column sums of d(gates), forward then reverse.
    ``mistake``: a key of MISTAKES, for the sensitivity test only."""
    assert mistake is None or mistake in MISTAKES
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    xf, xr = leaf(xg_f), leaf(xg_r)
    wf, wr = whh_f.detach().to(dtype), whh_r.detach().to(dtype)
    y, c, gf, gr, raw = lstm_seq_forward(xf, xr, wf, wr, lens, mistake)
    ((raw if mistake == 'd' else y) * dy.detach().to(dtype).reshape(y.shape)).sum().backward()
    dgf, dgr = xf.grad, xr.grad
    T, B, H4 = dgf.shape
    return dict(y=y.detach(), c=c.detach(), gates_f=gf.detach(), gates_r=gr.detach(), dgates_f=dgf, dgates_r=dgr,
                dbias=torch.stack([dgf.reshape(T * B, H4).sum(0), dgr.reshape(T * B, H4).sum(0)]))


def rnn_lens(B, T, gen):
    """Random in 1..T with lens[0] = T and, for B > 1, lens[B-1] = 1."""
    lens = torch.randint(1, T + 1, (B,), generator=gen)
    lens[0] = T
    if B > 1:
        lens[B - 1] = 1
    return [int(v) for v in lens]


def rnn_case(B, T, H, seed, lens=None):
    """xg ~ N(0,1), W_hh ~ N(0, 1/H) -- the recurrent term is as large as the input term, so a hand-off or packing defect moves the outputs
    at order 1 -- and dy ~ 0.3 N(0,1), all finite in the padded rows too (the GPU tests overwrite those of xg with NaN)."""
    g = torch.Generator().manual_seed(seed)
    xg = [rnd(g, T, B, 4 * H) for _ in range(2)]
    whh = [rnd(g, 4 * H, H, scale=H ** -0.5) for _ in range(2)]
    dy = rnd(g, T, B, 2 * H, scale=0.3)
    if lens is None:
        lens = rnn_lens(B, T, g)
    assert len(lens) == B and all(1 <= v <= T for v in lens)
    return dict(B=B, T=T, H=H, xg_f=xg[0], xg_r=xg[1], whh_f=whh[0], whh_r=whh[1], dy=dy, lens=lens)


def case_ref(case, dtype=torch.float64, mistake=None):
    return lstm_seq_ref(case['xg_f'], case['xg_r'], case['whh_f'], case['whh_r'], case['lens'], case['dy'], dtype, mistake)


# ---------------------------------------------------------------------------------------------
# one row per kernel form a 256-CU chip can reach: (B, H, T, switches, forward plan, backward plan); a plan is (family, a, b) in the
# parameter order of re2e_lstm_plan (b = None where the family has one parameter).  T = 7: an odd number of hand-offs, one-bit tags flip
# parity several times.  The switch rows name BOTH plans the library answers under their switches, not only the one they are there for.
# ---------------------------------------------------------------------------------------------
_P, _PB, _F2, _B3, _UW = 'RE2E_LSTM_PERSIST', 'RE2E_LSTM_PERSIST_BWD', 'RE2E_LSTM_FWD2', 'RE2E_LSTM_BWD3', 'RE2E_LSTM_BWD_UW'
RNN_SWITCHES = (_P, _PB, _F2, _B3, _UW)
RNN_CASES = [
    (3, 8, 7, {}, ('fwd_step', 1, None), ('bwd_persist', 1, 1)),
    (3, 64, 7, {}, ('fwd2_persist', 1, 1), ('bwd3', 8, 1)),
    (65, 64, 7, {}, ('fwd_persist', 4, 2), ('bwd3', 16, 1)),
    (3, 128, 7, {}, ('fwd2_persist', 1, 2), ('bwd3', 8, 2)),
    (33, 128, 7, {}, ('fwd_persist', 4, 4), ('bwd3', 16, 2)),
    (3, 144, 7, {}, ('fwd_step', 2, None), ('bwd_persist', 2, 1)),
    (3, 192, 7, {}, ('fwd_persist', 8, 3), ('bwd3', 8, 3)),
    (17, 192, 7, {}, ('fwd_persist', 8, 3), ('bwd3', 16, 3)),
    (3, 256, 7, {}, ('fwd2_persist', 1, 4), ('bwd3', 8, 4)),
    (17, 256, 7, {}, ('fwd_persist', 8, 4), ('bwd3', 16, 4)),
    (3, 288, 7, {}, ('fwd_step', 4, None), ('bwd_persist', 3, 1)),
    (3, 320, 7, {}, ('fwd2_persist', 2, 5), ('bwd3', 16, 5)),
    (17, 320, 7, {}, ('fwd_persist', 8, 5), ('bwd3', 16, 5)),
    (3, 384, 7, {}, ('fwd_step', 8, None), ('bwd3', 16, 6)),
    (3, 392, 7, {}, ('fwd_step', 1, None), ('bwd_persist', 4, 1)),
    (3, 448, 7, {}, ('fwd_step', 8, None), ('bwd3', 16, 7)),
    (3, 512, 7, {}, ('fwd2_persist', 2, 8), ('bwd3', 16, 8)),
    (17, 512, 7, {}, ('fwd2_persist', 4, 8), ('bwd3', 16, 8)),
    (65, 512, 7, {}, ('fwd2_step', 4, 8), ('bwd_persist', 4, 2)),
    (3, 640, 7, {}, ('fwd_step', 16, None), ('bwd_step', 2, None)),
    (129, 256, 4, {}, ('fwd_step', 8, None), ('bwd_step', 2, None)),          # the grid does not fit the chip: reached by shape alone
    (300, 104, 4, {}, ('fwd_step', 1, None), ('bwd_step', 1, None)),          # the same, at a width only the narrowest forms take
    (3, 64, 7, {_P: '0'}, ('fwd2_step', 1, 1), ('bwd3', 8, 1)),
    (3, 128, 7, {_P: '0'}, ('fwd2_step', 1, 2), ('bwd3', 8, 2)),
    (3, 256, 7, {_P: '0'}, ('fwd2_step', 1, 4), ('bwd3', 8, 4)),
    (3, 320, 7, {_P: '0'}, ('fwd2_step', 2, 5), ('bwd3', 16, 5)),
    (3, 512, 7, {_P: '0'}, ('fwd2_step', 2, 8), ('bwd3', 16, 8)),
    (3, 512, 7, {_F2: '0'}, ('fwd_persist', 8, 8), ('bwd3', 16, 8)),
    (3, 32, 7, {_PB: '0'}, ('fwd_persist', 4, 1), ('bwd_step', 1, None)),
    (3, 16, 7, {_UW: '2'}, ('fwd_step', 1, None), ('bwd_persist', 1, 2)),
    (3, 144, 7, {_UW: '2'}, ('fwd_step', 2, None), ('bwd_persist', 2, 2)),
    (17, 320, 7, {_B3: '0', _UW: '2'}, ('fwd_persist', 8, 5), ('bwd_persist', 3, 2)),
]


def case_id(row):
    B, H, T, env, fwd, bwd = row
    sw = ''.join('-%s=%s' % (k[len('RE2E_LSTM_'):], v) for k, v in sorted(env.items()))
    return 'B%d-H%d-T%d%s' % (B, H, T, sw)


def table_case(row):
    """The inputs of a row: a function of its shape alone, so rows that differ in their switches share inputs and reference."""
    B, H, T = row[:3]
    return rnn_case(B, T, H, seed=1000 * B + H + T)


def plan_key(plan):
    """A dict of re2e_lstm_plan -> (family, a, b) as RNN_CASES writes it."""
    order = {'fwd2_persist': ('tiles', 'nj'), 'fwd2_step': ('tiles', 'nj'), 'fwd_persist': ('waves', 'qn'), 'fwd_step': ('waves', None),
             'bwd3': ('un', 'tpw'), 'bwd_persist': ('tpw', 'uw'), 'bwd_step': ('jt', None)}
    ka, kb = order[plan['family']]
    return plan['family'], int(plan[ka]), int(plan[kb]) if kb else None
