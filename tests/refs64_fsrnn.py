"""Float64 reference of the fast-slow RNN window at its C-ABI contract (re2e_fsrnn_fwd / re2e_fsrnn_bwd, csrc/fsrnn.hip), of
re2e_lm_lstm_cell_zo, of the whole FS-RNN LM over one window, and the inputs of tests/test_fsrnn_kernels_gpu.py.

Plain torch on the CPU, autograd for the backward, nothing imported from the product or from ``oracle``; pinned to a chain of
``nn.LSTMCell`` in double and to tests/golden/fsrnn_tiny.npz by tests/test_refs64_fsrnn_cpu.py.  It takes ``dtype``: float64 is the
yardstick, the SAME code in float32 says how far fp32 arithmetic alone is from it on a given input (``margin_ok``).

The contract, restated (cell index 0 .. L-1 = fast cells, L = the slow cell; all cells are H wide; time-major):
  gates (L+1,T,B,4H)      gates[0] = x W_ih^T + b_ih + b_hh of fast cell 0 on entry (gate order i, f, g, o); every cell's activated gates after
                          the forward, d(pre-activations) after the backward
  hbuf, cbuf (L+1,T+1,B,H)  block t+1 of cell c = its state after zoneout at step t; block 0 of cells L-1 / L = the initial fast / slow state
  hd (2,T,B,H)            d1 . h of F0 and d2 . h of S (the inputs of S and F1), when dropout masks are given
  mh, mc (L+1,T,B,H)      zoneout masks: state = m . new + (1 - m) . old; a scalar keep instead of a tensor is the evaluation-mode blend
  dm (2,T,B,H)            the dropout masks d1, d2 (0 or 1 / (1 - p))
One step:  F0(pre; fast state) -> S(d1 . h; slow state) -> F1(d2 . h_S; fast state) -> F2 .. F(L-1)(no input; fast state); the output of the
step is the fast h after cell L-1.

``FS_CASES`` holds the shapes at which the cell-step kernels can go wrong: H = 1, 9, 33, 66 against k chunks of 32 and unit tiles of 16 /
32, B = 1, 3, 65 against the 64-row tile, T = 1, 2, 5, L = 2, 3, 4, the scalar blend against 0/1 masks, with and without the two dropout
masks, with and without a gradient through the final state, weights 4 bytes off a 16-byte boundary, and the recipe's H = 650.  The mask
keeps are 0.75 (h) and 0.5 (c), so that 1 - keep is exact in fp32.
"""
import torch

from refs64 import margin_ok, rel_err, rnd          # noqa: F401  (re-exported)

BAR_OUT = 1e-4          # states and activated gates, of the tensor's max
BAR_GRAD = 2e-4         # gradients, of the tensor's max
QUANTITIES = (('h', BAR_OUT), ('c', BAR_OUT), ('gates', BAR_OUT), ('hd', BAR_OUT), ('dgates', BAR_GRAD), ('d_fh0', BAR_GRAD), ('d_fc0', BAR_GRAD),
              ('d_sh0', BAR_GRAD), ('d_sc0', BAR_GRAD))
KEEP_H, KEEP_C, DROP_P = 0.75, 0.5, 0.5


def _cell(pre, c_prev):
    pi, pf, pg, po = pre.chunk(4, 1)
    gi, gf, gg, go = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
    c = gf * c_prev + gi * gg
    return go * torch.tanh(c), c, torch.cat([gi, gf, gg, go], 1)


def fs_window_forward(xg, W, state, mh, mc, dm, L, z=None):
    """The differentiable core, in the dtype of its inputs.  xg (T,B,4H); W: L+1 tuples (w_ih, w_hh, b_ih, b_hh) (cell 0's w_ih / biases and
    the w_ih of cells 2 .. L-1 are not used); state: (Fh, Fc, Sh, Sc) of (B,H); mh, mc: (L+1,T,B,H) tensors or Python floats; dm: (2,T,B,H)
    or None; z: optional (L+1,T,B,4H) added to the pre-activations (its gradient is d(pre-activations)).
    -> h, c (L+1,T,B,H), activated gates (L+1,T,B,4H), hd (2,T,B,H) or None."""
    T = xg.shape[0]
    Fh, Fc, Sh, Sc = state
    m = lambda M, c, t: M if isinstance(M, float) else M[c, t]
    hs, cs, gs = [[None] * T for _ in range(L + 1)], [[None] * T for _ in range(L + 1)], [[None] * T for _ in range(L + 1)]
    hd = [[None] * T, [None] * T]

    def run(c, t, pre, h_old, c_old):
        if z is not None:
            pre = pre + z[c, t]
        hn, cn, g = _cell(pre, c_old)
        a, b = m(mh, c, t), m(mc, c, t)
        h, cc = hn * a + (1 - a) * h_old, cn * b + (1 - b) * c_old
        hs[c][t], cs[c][t], gs[c][t] = h, cc, g
        return h, cc

    for t in range(T):
        Fh, Fc = run(0, t, xg[t] + Fh @ W[0][1].t(), Fh, Fc)
        x = Fh if dm is None else Fh * dm[0, t]
        hd[0][t] = x
        Sh, Sc = run(L, t, x @ W[L][0].t() + W[L][2] + W[L][3] + Sh @ W[L][1].t(), Sh, Sc)
        x = Sh if dm is None else Sh * dm[1, t]
        hd[1][t] = x
        Fh, Fc = run(1, t, x @ W[1][0].t() + W[1][2] + W[1][3] + Fh @ W[1][1].t(), Fh, Fc)
        for k in range(2, L):
            Fh, Fc = run(k, t, W[k][2] + W[k][3] + Fh @ W[k][1].t(), Fh, Fc)
    st = lambda rows: torch.stack([torch.stack(r) for r in rows])
    return st(hs), st(cs), st(gs), (st(hd) if dm is not None else None)


def fs_window_ref(xg, W, state, mh, mc, dm, L, dy, d_last=None, dtype=torch.float64):
    """What re2e_fsrnn_fwd / _bwd produce, as a dict of detached tensors: h, c (L+1,T,B,H) (blocks 1 .. T), gates, hd; dgates (L+1,T,B,4H)
    = d Loss / d pre-activations, d_fh0 .. d_sc0, and dW[c] = the gradients of (w_ih, w_hh, b_ih, b_hh) (None where unused), for
    Loss = sum(h[L-1] * dy) + sum over the final state of state * d_last (d_last: four (B,H) tensors or None)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    cv = lambda t: t if (t is None or isinstance(t, float)) else t.detach().to(dtype)
    T, B, H4 = xg.shape
    x = leaf(xg)
    st = [leaf(s) for s in state]
    Wl = [tuple(leaf(w) for w in cell) for cell in W]
    z = torch.zeros(L + 1, T, B, H4, dtype=dtype, requires_grad=True)
    h, c, g, hd = fs_window_forward(x, Wl, st, cv(mh), cv(mc), cv(dm), L, z)
    loss = (h[L - 1] * dy.detach().to(dtype)).sum()
    if d_last is not None:
        for s, d in zip((h[L - 1, -1], c[L - 1, -1], h[L, -1], c[L, -1]), d_last):
            loss = loss + (s * d.detach().to(dtype)).sum()
    loss.backward()
    dg = z.grad.clone()
    dg[0] = x.grad          # (the same thing: z[0] is added to xg)
    out = dict(h=h.detach(), c=c.detach(), gates=g.detach(), hd=hd.detach() if hd is not None else None, dgates=dg, d_fh0=st[0].grad, d_fc0=st[1].grad,
               d_sh0=st[2].grad, d_sc0=st[3].grad, y=h[L - 1].detach())
    out['dW'] = [tuple(w.grad for w in cell) for cell in Wl]
    return out


def fs_case(T, B, H, L, seed):
    """Pre-activations ~ N(0,1), weights ~ N(0, 1/H) (every product as large as its addend), biases ~ 0.3 N(0,1), a non-zero initial state,
    0/1 zoneout masks at keeps 0.75 / 0.5, dropout masks at p = 0.5 (0 or 2), gradients ~ 0.3 N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    W = [(rnd(g, 4 * H, H, scale=H ** -0.5), rnd(g, 4 * H, H, scale=H ** -0.5), rnd(g, 4 * H, scale=0.3), rnd(g, 4 * H, scale=0.3)) for _ in range(L + 1)]
    bern = lambda keep, *s: (torch.rand(*s, generator=g) < keep).float()
    return dict(T=T, B=B, H=H, L=L, xg=rnd(g, T, B, 4 * H), W=W,
                state=(torch.tanh(rnd(g, B, H)), rnd(g, B, H, scale=0.7), torch.tanh(rnd(g, B, H)), rnd(g, B, H, scale=0.7)),
                mh=bern(KEEP_H, L + 1, T, B, H), mc=bern(KEEP_C, L + 1, T, B, H), dm=bern(1 - DROP_P, 2, T, B, H) / (1 - DROP_P),
                dy=rnd(g, T, B, H, scale=0.3), d_last=tuple(rnd(g, B, H, scale=0.3) for _ in range(4)))


def case_ref(case, masks, drop, last, dtype=torch.float64):
    return fs_window_ref(case['xg'], case['W'], case['state'], case['mh'] if masks else KEEP_H, case['mc'] if masks else KEEP_C,
                         case['dm'] if drop else None, case['L'], case['dy'], case['d_last'] if last else None, dtype)


# (T, B, H, L, 0/1 zoneout masks (else the scalar blend), dropout masks, gradient through the final state (and of the initial state asked
# for), weights 4 bytes off a 16-byte boundary)
FS_H, FS_B, FS_T, FS_L = (1, 9, 33, 66), (1, 3, 65), (5, 2, 1), (2, 3, 4)
FS_CASES = [(FS_T[(i // 3 + i % 3) % 3], B, H, FS_L[(i // 3 + 2 * (i % 3)) % 3], i % 2 == 0, (i // 2) % 2 == 0, (i % 3 + i // 6) % 2 == 0, i % 4 == 1)
            for i, (H, B) in enumerate((H, B) for H in FS_H for B in FS_B)] + \
           [(2, 3, 650, 2, True, True, True, False), (2, 3, 650, 3, False, False, False, True)]
FS_PLANS = (('fsrnn_fwd_step', 64, 16), ('fsrnn_bwd_step', 64, 32))


def case_id(row):
    T, B, H, L, masks, drop, last, mis = row
    return 'T%d-B%d-H%d-L%d%s%s%s%s' % (T, B, H, L, '-masks' if masks else '-blend', '-drop' if drop else '', '-last' if last else '',
                                        '-misaligned' if mis else '')


def table_case(row):
    """The inputs of a row: a function of its shape alone."""
    T, B, H, L = row[:4]
    return fs_case(T, B, H, L, seed=7000 + 1000 * B + 10 * H + 100 * L + T)


def plan_key(plan):
    return plan['family'], int(plan['rows']), int(plan['units'])


# ---------------------------------------------------------------------------------------------
# re2e_lm_lstm_cell_zo
# ---------------------------------------------------------------------------------------------
def cell_zo_ref(x, w_ih, w_hh, b_ih, b_hh, h_prev, c_prev, keep_h, keep_c, dtype=torch.float64):
    """nn.LSTMCell + the evaluation-mode zoneout blend; x None: no input (b_ih still counts); h_prev / c_prev None: zeros -> (h, c)."""
    cv = lambda t: t.detach().to(dtype)
    n = (x if x is not None else h_prev if h_prev is not None else c_prev).shape[0] if (x is not None or h_prev is not None or c_prev is not None) else 1
    H = w_hh.shape[1]
    hp = cv(h_prev) if h_prev is not None else torch.zeros(n, H, dtype=dtype)
    cp = cv(c_prev) if c_prev is not None else torch.zeros(n, H, dtype=dtype)
    pre = cv(b_ih) + cv(b_hh) + hp @ cv(w_hh).t()
    if x is not None:
        pre = pre + cv(x) @ cv(w_ih).t()
    hn, cn, _ = _cell(pre, cp)
    return hn * keep_h + (1 - keep_h) * hp, cn * keep_c + (1 - keep_c) * cp


# ---------------------------------------------------------------------------------------------
# the whole model over one window: embedding -> d0 -> the fast-slow recurrence -> d3 -> output layer -> cross-entropy
# ---------------------------------------------------------------------------------------------
STATE_KEYS = ('F_h', 'F_c', 'S_h', 'S_c')


def param_names(L):
    cells = ['fast_cells.%d' % k for k in range(L)] + ['slow_cell']
    return ['embed.weight'] + ['%s.%s' % (c, n) for c in cells for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')] + ['out.weight', 'out.bias']


def fs_model_ref(params, xs, ts, L, keep_h, keep_c, state=None, masks=None, dtype=torch.float64):
    """params: name -> tensor (param_names(L)); xs, ts (T,B) labels and targets; state: {'F_h','F_c','S_h','S_c'} or None (zeros); masks: None
    (evaluation mode: the blend, no dropout) or a dict with d0 (T,B,E), d1, d2, d3 (T,B,H) multiplicative dropout masks (or None each) and mh, mc
    (L+1,T,B,H) 0/1 zoneout masks (or a float) -> dict: losses (T,), loss, logits, the final state, grad.<name> (fast_cells.k>=2.weight_ih: zeros)."""
    names = param_names(L)
    P = {k: params[k].detach().to(dtype).clone().requires_grad_(True) for k in names}
    xs, ts = torch.as_tensor(xs).long(), torch.as_tensor(ts).long()
    T, B = xs.shape
    H = P['slow_cell.weight_hh'].shape[1]
    st = tuple(state[k].detach().to(dtype) if state is not None else torch.zeros(B, H, dtype=dtype) for k in STATE_KEYS)
    masks = masks or {}
    cv = lambda v: v if (v is None or isinstance(v, float)) else torch.as_tensor(v).to(dtype)
    d = [cv(masks.get('d%d' % i)) for i in range(4)]
    mh, mc = cv(masks.get('mh', float(keep_h))), cv(masks.get('mc', float(keep_c)))
    cells = ['fast_cells.%d' % k for k in range(L)] + ['slow_cell']
    W = [tuple(P['%s.%s' % (c, n)] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')) for c in cells]
    x = P['embed.weight'][xs]
    if d[0] is not None:
        x = x * d[0].reshape(x.shape)
    xg = x @ W[0][0].t() + W[0][2] + W[0][3]
    dm = torch.stack([d[1].reshape(T, B, H), d[2].reshape(T, B, H)]) if d[1] is not None else None
    h, c, _, _ = fs_window_forward(xg, W, st, mh, mc, dm, L)
    y = h[L - 1]
    if d[3] is not None:
        y = y * d[3].reshape(y.shape)
    logits = y @ P['out.weight'].t() + P['out.bias']
    losses = torch.stack([torch.nn.functional.cross_entropy(logits[t], ts[t]) for t in range(T)])
    loss = losses.sum()
    loss.backward()
    out = dict(losses=losses.detach(), loss=loss.detach(), logits=logits.detach(), F_h=h[L - 1, -1].detach(), F_c=c[L - 1, -1].detach(), S_h=h[L, -1].detach(),
               S_c=c[L, -1].detach())
    out.update({'grad.' + k: (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])) for k in names})
    return out
