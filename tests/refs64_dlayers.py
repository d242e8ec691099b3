"""Float64 reference of the multi-layer attention decoder (dlayers > 1; csrc/decstack.hip, ops.DecoderUpperFn, ops.DecoderLoopFn with
``upper``) and the inputs of tests/test_decstack_kernels_gpu.py.

Plain torch on the CPU, autograd for every gradient, nothing imported from the product or from ``oracle``.  Layer 0 is the loop of
refs64.decoder_loop_ref (``location``) or refs64_att.att_loop_ref (the other kinds); ``upper_ref`` stacks the layers above on its states,
written out from the formula; ``upper_modules`` is a second derivation through torch.nn.LSTMCell.  The attention reads layer 0 only, so
a loop with sampled tokens is the teacher-forced loop on the tokens that were fed (integers: no gradient through the choice) --
``sampled_tokens`` replays the choice from the top layer's states to check which tokens those are."""
import torch

import refs64 as R
import refs64_att as RA

UPPER_KEYS = ('w_ih', 'w_hh', 'b_ih', 'b_hh')


def upper_ref(z0, layers):
    """z0 (L1,B,D) states of layer 0, layers: list of dicts w_ih (4D,D), w_hh (4D,D), b_ih, b_hh (4D) from layer 1 up -> list of the layers'
    states (L1,B,D), the last one the top.  Layer l, token i, with z_l[-1] = c_l[-1] = 0 (torch gate order i, f, g, o):
        gates = w_ih z_{l-1}[i] + b_ih + w_hh z_l[i-1] + b_hh;  c_l[i] = sigmoid(f) c_l[i-1] + sigmoid(i) tanh(g);  z_l[i] = sigmoid(o) tanh(c_l[i])"""
    L1, B, D = z0.shape
    below, outs = z0, []
    for lay in layers:
        z, c = z0.new_zeros(B, D), z0.new_zeros(B, D)
        bias = lay['b_ih'] + lay['b_hh']
        zs = []
        for i in range(L1):
            gi, gf, gg, go = (below[i] @ lay['w_ih'].t() + z @ lay['w_hh'].t() + bias).chunk(4, 1)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            z = torch.sigmoid(go) * torch.tanh(c)
            zs.append(z)
        below = torch.stack(zs, 0)
        outs.append(below)
    return outs


def upper_modules(z0, layers):
    """The same stack through torch.nn.LSTMCell modules holding the layers' tensors, token-major as the reference runs it (all layers of
    token i before token i + 1) -> (top states, list of dicts of the modules' parameters)."""
    L1, B, D = z0.shape
    cells, params = [], []
    for lay in layers:
        cell = torch.nn.LSTMCell(D, D).to(z0.dtype)
        for n, k in (('weight_ih', 'w_ih'), ('weight_hh', 'w_hh'), ('bias_ih', 'b_ih'), ('bias_hh', 'b_hh')):
            getattr(cell, n).data.copy_(lay[k])
        cells.append(cell)
        params.append(dict(w_ih=cell.weight_ih, w_hh=cell.weight_hh, b_ih=cell.bias_ih, b_hh=cell.bias_hh))
    state = [(z0.new_zeros(B, D), z0.new_zeros(B, D)) for _ in layers]
    top = []
    for i in range(L1):
        x = z0[i]
        for l, cell in enumerate(cells):
            state[l] = cell(x, state[l])
            x = state[l][0]
        top.append(x)
    return torch.stack(top, 0), params


def layer0_ref(kind, hmask, pre, ids, hlens, L1, Pm):
    """The teacher-forced loop of layer 0 on the tokens ``ids`` -> (z0 (L1,B,D), w (L1,B,T))."""
    if kind == 'location':
        return R.decoder_loop_ref(hmask, pre, ids, hlens, L1, Pm)
    zs, w, _ = RA.att_loop_ref(kind, hmask, pre, ids, hlens, L1, Pm)
    return zs, w


def sampled_tokens(z_top, ids, out_w, out_b, sample_steps):
    """The tokens a loop with ``sample_steps`` feeds, given the top layer's states of the loop that fed them: step i > 0 with sample_steps[i]
    feeds the arg-max (lowest index) of output(z_top[i-1]) -> (tokens (L1,B), smallest margin between the two best logits at a sampled step)."""
    fed, margin = ids.clone(), float('inf')
    for i in range(1, ids.shape[0]):
        if sample_steps[i]:
            logits = (z_top[i - 1] @ out_w.t() + out_b).detach()
            fed[i] = R.argmax_first(logits).to(ids.dtype)
            top2 = logits.topk(2, dim=1).values
            margin = min(margin, float((top2[:, 0] - top2[:, 1]).min()))
    return fed, margin


# (B, L1, D, layers) and why the shape is here.  The kernels' break points: 8 rows and 4 hidden units (forward) / 4 output units (backward) per
# workgroup, a 256-float stride of the contraction (64 lanes x float4) over D (forward) and over 4D (backward).
STACK_SHAPES = [
    ((1, 1, 4, 2), 'one of everything: no recurrence'),
    ((2, 3, 300, 2), 'the default width, a multiple of 4 but not of 8; D one lane pass plus 11 lanes'),
    ((5, 6, 12, 3), 'three layers, six steps of carry'),
    ((32, 2, 320, 2), 'the persistent loop\'s row limit: four full row tiles'),
    ((33, 2, 68, 2), 'one past it: a row tile of one row; D = 4 * 17: an odd number of unit groups'),
    ((3, 4, 132, 2), 'D one float4 past a 128 tile'),
    ((9, 2, 260, 2), 'one row past a row tile of 8 and D one float4 past the 256-float stride of the forward contraction'),
    ((2, 2, 20, 2), '4D = 80: the backward contraction shorter than one 256-float stride, five unit groups'),
]
# the layer-0 loop around the stack: (T, E, A, C, Fh), small and inside the persistent form's limits where B and D are
LOOP_DIMS = (40, 64, 64, 12, 100)


def stack_case(shape):
    """z0, upstream gradient and the layers' parameters at the weight scales of refs64.decoder_case."""
    B, L1, D, nl = shape
    g = torch.Generator().manual_seed(B * 1000 + L1 * 100 + D + nl)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    layers = [dict(w_ih=r(4 * D, D, scale=0.08), w_hh=r(4 * D, D, scale=0.08), b_ih=r(4 * D, scale=0.1), b_hh=r(4 * D, scale=0.1)) for _ in range(nl - 1)]
    return dict(z0=torch.tanh(r(L1, B, D)) * 0.8, gz=r(L1, B, D), layers=layers, L1=L1)


def stack_ref_run(case, dtype=torch.float64, stack=upper_ref):
    """upper_ref and its gradients under the case's upstream gradient -> dict: z_top, dZ0, and ``l<k>.<key>`` for every parameter of layer k."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    z0 = leaf(case['z0'])
    layers = [{k: leaf(v) for k, v in lay.items()} for lay in case['layers']]
    if stack is upper_ref:
        top, grads_of = upper_ref(z0, layers)[-1], layers
    else:
        top, grads_of = upper_modules(z0, layers)
    (top * case['gz'].to(dtype)).sum().backward()
    out = dict(z_top=top.detach(), dZ0=z0.grad)
    for l, lay in enumerate(grads_of):
        out.update({'l%d.%s' % (l + 1, k): lay[k].grad for k in UPPER_KEYS})
    return out


def loop_case(shape):
    """The full stacked loop: refs64.decoder_case on (B, T, L1, E, A, D, C, Fh) with LOOP_DIMS plus the stack_case layers."""
    B, L1, D, nl = shape
    T, E, A, C, Fh = LOOP_DIMS
    c = dict(R.decoder_case((B, T, L1, E, A, D, C, Fh)))
    c['layers'] = stack_case(shape)['layers']
    c['kind'] = 'location'
    return c


def loop_ref_run(case, dtype=torch.float64, upstream='zs'):
    """layer0_ref + upper_ref and their gradients under gz on the TOP states (and gw on the attention weights) -> dict: z_top, w, d_enc, d_pre,
    every Pm key, ``l<k>.<key>``."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    hm, pr = leaf(case['hmask']), leaf(case['pre'])
    Pm = {k: leaf(v) for k, v in case['Pm'].items()}
    layers = [{k: leaf(v) for k, v in lay.items()} for lay in case['layers']]
    z0, w = layer0_ref(case['kind'], hm, pr, case['ids'], case['hlens'], case['L1'], Pm)
    top = upper_ref(z0, layers)[-1] if layers else z0
    assert upstream in R.DEC_UPSTREAM
    up = (top * case['gz'].to(dtype)).sum()
    if upstream == 'zs+w':
        up = up + (w * case['gw'].to(dtype)).sum()
    up.backward()
    out = dict(z_top=top.detach(), w=w.detach(), d_enc=hm.grad, d_pre=pr.grad)
    out.update({k: v.grad for k, v in Pm.items()})
    for l, lay in enumerate(layers):
        out.update({'l%d.%s' % (l + 1, k): lay[k].grad for k in UPPER_KEYS})
    return out
