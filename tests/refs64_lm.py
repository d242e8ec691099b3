"""Float64 reference of the language model's recurrence at its C-ABI contract (re2e_lmseq_fwd / re2e_lmseq_bwd, csrc/lmseq.hip) -- one
truncated-BPTT window of a unidirectional LSTM whose state is carried in and out -- of re2e_sgd_step, and the inputs of
tests/test_lmseq_kernels_gpu.py.

Plain torch on the CPU, autograd for the backward, nothing imported from the product or from ``oracle``; pinned to a chain of
``nn.LSTMCell`` in double by tests/test_refs64_lm_cpu.py.  Like the other references it takes ``dtype``: float64 is the yardstick, the SAME
code in float32 says how far fp32 arithmetic alone is from it on a given input (``margin_ok``).

``LM_CASES`` holds the shapes at which the step kernels can go wrong: K and unit-tile remainders (H = 1, 9, 10, 33, 66 against k chunks
of 32 and unit tiles of 16 / 32), odd H (rows of W_hh that are only 4-byte aligned), the recipe's H = 650, partial row tiles on both sides
of the 64-row tile (B = 1, 3, 33, 65), one, two and five steps, with and without a gradient through the final state, with and without the
gradient of the initial state asked for, and W_hh 4 bytes off a 16-byte boundary.  tests/test_refs64_lm_cpu.py checks that the table is
closed under re2e_lmseq_plan.
"""
import torch

from refs64 import margin_ok, rel_err, rnd          # noqa: F401  (re-exported)

# the project's own bars (tests/refs64_rnn.py, from test_kernels_gpu.py: test_bilstm)
BAR_OUT = 1e-4          # h, c and the activated gates, of the tensor's max
BAR_GRAD = 2e-4         # d(pre-activation gates), dh0, dc0, of the tensor's max
QUANTITIES = (('h', BAR_OUT), ('c', BAR_OUT), ('gates', BAR_OUT), ('dgates', BAR_GRAD), ('dh0', BAR_GRAD), ('dc0', BAR_GRAD))


def lm_window_forward(xg, whh, h0, c0):
    """The differentiable core, in the dtype of its inputs: xg (T,B,4H) = x W_ih^T + b_ih + b_hh in gate order i, f, g, o; whh (4H,H);
    h0, c0 (B,H) -> (h (T,B,H), c (T,B,H), activated gates (T,B,4H))."""
    h, c = h0, c0
    hs, cs, gs = [], [], []
    for t in range(xg.shape[0]):
        pi, pf, pg, po = (xg[t] + h @ whh.t()).chunk(4, 1)
        gi, gf, gg, go = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
        c = gf * c + gi * gg
        h = go * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        gs.append(torch.cat([gi, gf, gg, go], 1))
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def lm_window_ref(xg, whh, h0, c0, dy, dh_last=None, dc_last=None, dtype=torch.float64):
    """What re2e_lmseq_fwd / _bwd produce, as a dict of detached tensors: h, c (T,B,H) (blocks 1 .. T of hbuf / cbuf), gates (T,B,4H)
    activated; dgates (T,B,4H) = d L / d pre-activations, dh0, dc0 (B,H) = d L / d initial state, for
    L = sum(h * dy) + sum(h[T-1] * dh_last) + sum(c[T-1] * dc_last)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    x, h0_, c0_ = leaf(xg), leaf(h0), leaf(c0)
    h, c, g = lm_window_forward(x, whh.detach().to(dtype), h0_, c0_)
    L = (h * dy.detach().to(dtype)).sum()
    if dh_last is not None:
        L = L + (h[-1] * dh_last.detach().to(dtype)).sum()
    if dc_last is not None:
        L = L + (c[-1] * dc_last.detach().to(dtype)).sum()
    L.backward()
    return dict(h=h.detach(), c=c.detach(), gates=g.detach(), dgates=x.grad, dh0=h0_.grad, dc0=c0_.grad)


def lm_case(T, B, H, seed):
    """xg ~ N(0,1), W_hh ~ N(0, 1/H): the recurrent term is as large as the input term, so a tiling or remainder defect moves the outputs
    at order 1; a non-zero initial state (|h0| < 1 as an LSTM output is); dy, dh_last, dc_last ~ 0.3 N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    return dict(T=T, B=B, H=H, xg=rnd(g, T, B, 4 * H), whh=rnd(g, 4 * H, H, scale=H ** -0.5), h0=torch.tanh(rnd(g, B, H)), c0=rnd(g, B, H, scale=0.7),
                dy=rnd(g, T, B, H, scale=0.3), dh_last=rnd(g, B, H, scale=0.3), dc_last=rnd(g, B, H, scale=0.3))


def case_ref(case, last=True, dtype=torch.float64):
    return lm_window_ref(case['xg'], case['whh'], case['h0'], case['c0'], case['dy'], case['dh_last'] if last else None,
                         case['dc_last'] if last else None, dtype)


# (T, B, H, gradient through the final state given, gradient of the initial state asked for, W_hh 4 bytes off a 16-byte boundary)
LM_H, LM_B, LM_T = (1, 9, 10, 33, 66), (1, 3, 33, 65), (5, 2, 1)
LM_CASES = [(LM_T[i % 3], B, H, i % 2 == 0, (i // 2) % 2 == 0, i % 4 == 1)
            for i, (H, B) in enumerate((H, B) for H in LM_H for B in LM_B)] + [(2, 3, 650, True, True, False), (2, 3, 650, False, True, True)]
# the one form per direction the plan names: (family, rows, units) of every case
LM_PLANS = (('fwd_step', 64, 16), ('bwd_step', 64, 32))


def case_id(row):
    T, B, H, last, out, mis = row
    return 'T%d-B%d-H%d%s%s%s' % (T, B, H, '-last' if last else '', '-dstate' if out else '', '-misaligned' if mis else '')


def table_case(row):
    """The inputs of a row: a function of its shape alone."""
    T, B, H = row[:3]
    return lm_case(T, B, H, seed=4000 + 1000 * B + 10 * H + T)


def plan_key(plan):
    return plan['family'], int(plan['rows']), int(plan['units'])


def sgd_ref(p, g, lr, stats, dtype=torch.float64):
    """re2e_sgd_step: p - lr * stats[1] * g, or p unchanged when stats[2] == 0."""
    if float(stats[2]) == 0.0:
        return p.detach().to(dtype).clone()
    return p.detach().to(dtype) - torch.as_tensor(lr, dtype=dtype) * stats[1].detach().to(dtype) * g.detach().to(dtype)


# ---------------------------------------------------------------------------------------------
# the whole model over one window: embedding -> d0 -> LSTM 1 -> d1 -> LSTM 2 -> d2 -> output layer -> cross-entropy
# ---------------------------------------------------------------------------------------------
PARAM_NAMES = ('embed.weight', 'l1.weight_ih', 'l1.weight_hh', 'l1.bias_ih', 'l1.bias_hh', 'l2.weight_ih', 'l2.weight_hh', 'l2.bias_ih', 'l2.bias_hh',
               'lo.weight', 'lo.bias')
STATE_KEYS = ('c1', 'h1', 'c2', 'h2')


def lm_model_ref(params, xs, ts, state=None, masks=None, dtype=torch.float64):
    """params: name -> tensor (PARAM_NAMES); xs, ts (T,B) integer labels and targets; state: {'c1','h1','c2','h2'} of (B,H) or None
    (zeros); masks: None or three tensors, the multiplicative dropout masks (0 or 1/(1-p)) of the (T,B,I), (T,B,H) and (T,B,H) tensors
    behind the embedding, layer 1 and layer 2 -> dict: losses (T,) = mean cross-entropy of each step, loss = their sum, the final state,
    grad.<name> = d loss / d parameter, logits (T,B,V)."""
    P = {k: params[k].detach().to(dtype).clone().requires_grad_(True) for k in PARAM_NAMES}
    xs, ts = torch.as_tensor(xs).long(), torch.as_tensor(ts).long()
    T, B = xs.shape
    H = P['l1.weight_hh'].shape[1]
    st = {k: (state[k].detach().to(dtype) if state is not None else torch.zeros(B, H, dtype=dtype)) for k in STATE_KEYS}
    m = [torch.as_tensor(v).to(dtype) for v in masks] if masks is not None else [None] * 3
    drop = lambda x, k: x if m[k] is None else x * m[k].reshape(x.shape)
    x = drop(P['embed.weight'][xs], 0)                                                      # (T,B,I)
    h1, c1, _ = lm_window_forward(x @ P['l1.weight_ih'].t() + P['l1.bias_ih'] + P['l1.bias_hh'], P['l1.weight_hh'], st['h1'], st['c1'])
    h2, c2, _ = lm_window_forward(drop(h1, 1) @ P['l2.weight_ih'].t() + P['l2.bias_ih'] + P['l2.bias_hh'], P['l2.weight_hh'], st['h2'], st['c2'])
    logits = drop(h2, 2) @ P['lo.weight'].t() + P['lo.bias']
    losses = torch.stack([torch.nn.functional.cross_entropy(logits[t], ts[t]) for t in range(T)])
    loss = losses.sum()
    loss.backward()
    out = dict(losses=losses.detach(), loss=loss.detach(), logits=logits.detach(), c1=c1[-1].detach(), h1=h1[-1].detach(), c2=c2[-1].detach(), h2=h2[-1].detach())
    out.update({'grad.' + k: P[k].grad for k in PARAM_NAMES})
    return out
