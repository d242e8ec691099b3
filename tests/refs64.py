"""Float64 references of the loss-side operations (csrc/ctc.hip, seqloss.hip, attloc.hip, decloop.hip) and the inputs of
tests/test_loss_kernels_gpu.py.

Plain torch on the CPU, autograd for every gradient, nothing imported from the product or from ``oracle``: the references here are
second derivations (CTC: torch's own ``F.ctc_loss`` on doubles; the decoder loop: written out from the formula in the header of
csrc/attloc.hip), pinned to the reference-made golden vectors by tests/test_refs64_cpu.py.

Every reference takes ``dtype``.  float64 is the yardstick; the SAME code in float32 says how far fp32 arithmetic alone is from it
on a given input, which is what makes a tolerance meaningful (``margin_ok``): an input on which torch's own fp32 run uses up the
bar would turn a failure into noise.
"""
import math

import torch
import torch.nn.functional as F

# the project's own bars (tests/test_kernels_gpu.py: test_ctc, test_decoder_loop_persistent_vs_stepwise and its backward twin)
BAR_LOSS = 1e-5            # CTC / CE / label-smoothing loss, relative
BAR_GRAD = 1e-4            # their gradients (and log_softmax rows), of the tensor's max
BAR_DEC_OUT = 2e-4         # decoder states and attention weights over the whole loop, of the tensor's max
BAR_DEC_GRAD = 3e-4        # decoder gradients: 3e-4 * scale + 1e-7
ATOL_DEC_GRAD = 1e-7


def rel_err(got, ref):
    """max |got - ref| / max |ref| over the FINITE entries of ref (1.0 where ref is all zero and got is not)."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = torch.isfinite(ref)
    if not fin.any():
        return 0.0
    err = (got[fin] - ref[fin]).abs().max().item()
    scale = ref[fin].abs().max().item()
    if not math.isfinite(err):
        return float('inf')
    if scale == 0.0:
        return 0.0 if err == 0.0 else 1.0
    return err / scale


def margin_ok(name, f32, f64, bar, atol=0.0):
    """Precondition of a bar: the fp32 CPU run of the same reference stays within a quarter of it.  Returns the fp32 error."""
    e = rel_err(f32, f64)
    scale = f64.detach().double().abs().max().item() if f64.numel() else 0.0
    lim = 0.25 * bar + (0.25 * atol / scale if scale > 0 else 0.0)
    assert e <= lim, 'input too hard for the bar: fp32 CPU reference of %s is %.3e from float64, the bar is %.1e' % (name, e, bar)
    return e


def rnd(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


# ---------------------------------------------------------------------------------------------
# CTC
# ---------------------------------------------------------------------------------------------
def ctc_ref(logits, hlens, labels, dtype=torch.float64):
    """logits (T,B,V) raw activations, hlens list, labels list of lists -> (nll per utterance (B,), loss = sum / B, d loss / d logits).
    Softmax inside, blank 0.  An utterance whose frames cannot carry its labels has nll = +inf and NaN gradient rows."""
    T, B, V = logits.shape
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    flat = torch.tensor([v for l in labels for v in l], dtype=torch.long)
    nll = F.ctc_loss(x.log_softmax(2), flat, torch.tensor(hlens, dtype=torch.long), torch.tensor([len(l) for l in labels], dtype=torch.long),
                     blank=0, reduction='none', zero_infinity=False)
    loss = nll.sum() / B
    loss.backward()
    return nll.detach(), loss.detach(), x.grad


def min_frames(label):
    """Frames an alignment of ``label`` needs: its length plus one blank between equal neighbours."""
    return len(label) + sum(1 for a, b in zip(label, label[1:]) if a == b)


def _ctc_case(name, T, V, hlens, labels, seed, scale=2.0, gscale=1.3, ldd=None, boost=0.0):
    """``boost``: added to the logit of the symbol an evenly spread alignment emits at each frame.  With dozens of random labels on random
    logits the likelihood is e^-400 and alpha + beta + nll cancels to a few digits in fp32 (torch's own fp32 gradient is then 1e-4 of
    its max from float64); along a plausible alignment the nll is a few tens, as for a model that has learnt something."""
    g = torch.Generator().manual_seed(seed)
    B = len(hlens)
    assert max(hlens) <= T and len(labels) == B and all(0 < v < V for l in labels for v in l)
    logits = rnd(g, T, B, V, scale=scale)
    if boost:
        for b, (h, l) in enumerate(zip(hlens, labels)):
            Sb = 2 * len(l) + 1
            for t in range(h):
                s = t * Sb // h
                logits[t, b, l[s >> 1] if s & 1 else 0] += boost
    return dict(name=name, T=T, B=B, V=V, hlens=hlens, labels=labels, logits=logits, gscale=gscale, ldd=ldd)


def _rand_labels(gen, n, V):
    return [int(v) for v in torch.randint(1, V, (n,), generator=gen)]


def ctc_cases():
    """name -> case; every alignment here is feasible (``ctc_infeasible_case`` is the one that is not)."""
    cs = []
    # all four log-sum-exp kernels and both sides of each threshold (V <= 512 / 1536 / 4608); T*B = 27 rows: a row tail in the 4-row workgroups
    for V in (17, 512, 513, 1536, 1537, 4608, 4609):
        cs.append(_ctc_case('widths-V%d' % V, 9, V, [9, 7, 5], [[1, 2, 2, V - 1], [V - 1, 3], [5]], seed=100 + V, gscale=0.7))
    g = torch.Generator().manual_seed(7)
    # S = 65 / 63: two wavefronts in ctc_alpha_beta (the first hand-off that needs its barriers), second trip of the gather loop
    cs.append(_ctc_case('two-wavefronts', 70, 37, [70, 66], [_rand_labels(g, 32, 37), _rand_labels(g, 31, 37)], seed=201, scale=1.0, boost=6.0))
    # S = 131 / 129: three wavefronts, second trip of ctc_grad's odd-state loop (s += 128)
    cs.append(_ctc_case('three-wavefronts', 140, 37, [140, 135], [_rand_labels(g, 65, 37), _rand_labels(g, 64, 37)], seed=202, scale=1.0, boost=6.0))
    # skip_in / skip_out, first-occurrence scan and same-label sum of ctc_grad
    cs.append(_ctc_case('repeats', 40, 11, [40, 33, 25], [[4] * 6, [1, 2, 1, 2, 1, 2], [1, 2, 3, 4, 5, 6]], seed=203, gscale=2.5, boost=4.0))
    # hlen == L + repeats: exactly one path, the occupancy is one-hot per frame
    cs.append(_ctc_case('single-path', 6, 7, [4, 6, 3], [[3, 3, 5], [1, 2, 3, 4, 5, 6], [2, 2]], seed=204, gscale=0.5))
    # Sb = 1 beside Sb = 11 in one batch
    cs.append(_ctc_case('empty-beside-L5', 12, 9, [12, 9, 4], [[], [1, 2, 3, 4, 5], []], seed=205))
    # one frame: the t = 1.. loops are never entered (L = 0 and L = 1)
    cs.append(_ctc_case('one-frame', 3, 6, [3, 1, 1], [[2], [], [4]], seed=206, gscale=1.7))
    # rows of ldd > V floats, called through the C ABI
    cs.append(_ctc_case('padded-rows', 9, 37, [9, 6, 4], [[5, 5, 36], [1], [7, 8]], seed=207, ldd=48))
    for c in cs:
        assert all(min_frames(l) <= h for l, h in zip(c['labels'], c['hlens'])), c['name']
    assert all(min_frames(l) == h for l, h in zip(cs[10]['labels'], cs[10]['hlens'])) and cs[10]['name'] == 'single-path'
    return {c['name']: c for c in cs}


def ctc_infeasible_case():
    """[2,2,2] needs 5 frames and has 3; four labels in 3 frames; beside two feasible utterances."""
    c = _ctc_case('infeasible', 8, 7, [8, 3, 5, 3], [[1, 2], [2, 2, 2], [3], [1, 2, 3, 4]], seed=208)
    c['infeasible'] = [1, 3]
    return c


# ---------------------------------------------------------------------------------------------
# seqloss: cross-entropy with ignore, label smoothing, embedding gradient, row log-softmax / arg-max
# ---------------------------------------------------------------------------------------------
def argmax_first(x):
    """Arg-max of each row, the LOWEST index among equal maxima (ce_rows_kernel, argmax_rows_kernel)."""
    V = x.shape[1]
    eq = x == x.max(1, keepdim=True).values
    return torch.where(eq, torch.arange(V).expand_as(x), torch.full_like(eq, V, dtype=torch.long)).min(1).values


def ce_ref(logits, targets, scale, dtype=torch.float64):
    """(R,V) logits, targets (R,) with -1 = ignore -> (scale * mean over valid rows of -log_softmax[target], #correct, #valid, d loss / d logits)."""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    tg = targets.long()
    valid = tg >= 0
    lsm = x.log_softmax(1)
    loss = scale * (-lsm[valid, tg[valid]]).sum() / valid.sum()
    loss.backward()
    correct = int(((argmax_first(x.detach()) == tg) & valid).sum())
    return loss.detach(), correct, int(valid.sum()), x.grad


def lsm_ref(logits, dist, nutt, dtype=torch.float64):
    """-(1/nutt) * sum over ALL rows of log_softmax(logits) * dist -> (value, d value / d logits)."""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    reg = -(x.log_softmax(1) * dist.to(dtype)).sum() / nutt
    reg.backward()
    return reg.detach(), x.grad


def embedding_bwd_ref(dout, ids, V, beta=0.0, prev=None, dtype=torch.float64):
    """Gradient of the (V,D) table under ``dout`` (n,D) on the gathered rows, plus beta * prev."""
    table = torch.zeros(V, dout.shape[1], dtype=dtype, requires_grad=True)
    F.embedding(ids.long(), table).backward(dout.to(dtype))
    return table.grad + (beta * prev.to(dtype) if beta != 0.0 else 0.0)


SEQLOSS_SHAPES = [(5, 7), (13, 64), (13, 65), (6, 4233)]      # one lane pass, exactly one full pass, one past it, the production vocabulary


def seqloss_case(R, V):
    """Logits with everything cross-entropy can get wrong: a third of the rows ignored, a tie for the maximum whose lower / higher index
    is the target (two rows the lower, one the higher), a row around +-80 (the max subtraction), the last column as a target; a ``dist`` with exact zeros that does not sum to 1."""
    g = torch.Generator().manual_seed(1000 * R + V)
    x = rnd(g, R, V, scale=2.0)
    tg = torch.randint(0, V, (R,), generator=g)
    tg[1::3] = -1
    x[0, 1], x[0, V - 2] = 12.0, 12.0                # tie at 1 and V-2, target the lower one: counted as correct
    tg[0] = 1
    x[2, 0], x[2, V - 1] = 11.5, 11.5                # tie at 0 and V-1, target the higher one: NOT correct (lowest index wins)
    tg[2] = V - 1
    x[3] = rnd(g, V, scale=1.0) + torch.where(torch.arange(V) % 2 == 0, 80.0, -80.0)
    x[3, 0], x[3, 4] = 85.0, 85.0                   # a second tie with the lower index as the target: a flipped rule changes the COUNT,
    tg[3] = 0                                       # and does not just move one correct row from here to row 2
    dist = torch.rand(V, generator=g) * (2.0 / V)
    dist[::3] = 0.0
    return dict(x=x, targets=tg.to(torch.int32), scale=3.25, g=0.6, dist=dist, nutt=max(1, R // 2) + 1)


EMB_CASES = [(n, D) for n in (1, 63, 64, 65, 200) for D in (4, 14, 300)]


def embedding_case(n, D):
    """ids over a 9-row table: row 3 is hit by more than half of the positions (> 64 times and in every ballot pass at n = 200), rows 7
    and 8 never; dout rows of ldo = D + 3 floats."""
    g = torch.Generator().manual_seed(17 * n + D)
    V, ldo = 9, D + 3
    ids = torch.randint(0, 7, (n,), generator=g)
    ids[torch.rand(n, generator=g) < 0.55] = 3
    ids[n - 1] = 3
    dout = rnd(g, n, ldo)
    prev = rnd(g, V, D)
    return dict(V=V, ldo=ldo, ids=ids.to(torch.int32), dout=dout, prev=prev)


# ---------------------------------------------------------------------------------------------
# decoder loop: AttLoc step -> LSTMCell, teacher forced (what ops.DecoderLoopFn computes)
# ---------------------------------------------------------------------------------------------
def decoder_loop_ref(hmask, pre, ids, hlens, L1, Pm):
    """hmask (B,T,E) encoder states (zero beyond hlens), pre (B,T,A) their attention projection, ids (L1,B) tokens fed, Pm: embed (V,Dd),
    w_ih (4D,Dd+E), w_hh (4D,D), b_ih, b_hh (4D), mlp_dec (A,D), mlp_att (A,C), loc_conv (C,1,1,2Fh+1), gvec_w (1,A), gvec_b (1)
    -> (zs (L1,B,D), w (L1,B,T)) in the dtype of its inputs; differentiable.

    Step i, with z_0 = c_0 = 0 and w_{-1}[b,t] = 1/hlen_b for t < hlen_b, else 0:
        conv[b,t,c] = sum_k w_{i-1}[b, t + k - Fh] * loc_conv[c,k]                       (zero outside 0..T-1)
        e[b,t]      = gvec . tanh(mlp_att conv[b,t] + pre[b,t] + mlp_dec z_i[b]) + gvec_b
        w_i[b,:]    = softmax over ALL T frames of 2 * e[b,:]
        ctx[b]      = sum_t w_i[b,t] hmask[b,t]
        gates       = w_ih [embed[ids[i,b]] | ctx[b]] + b_ih + w_hh z_i[b] + b_hh            (i, f, g, o)
        c_{i+1}     = sigmoid(f) c_i + sigmoid(i) tanh(g);   z_{i+1} = sigmoid(o) tanh(c_{i+1})
    """
    B, T, E = hmask.shape
    D = Pm['w_hh'].shape[1]
    C, Kf = Pm['loc_conv'].shape[0], Pm['loc_conv'].shape[3]
    Fh = (Kf - 1) // 2
    taps = Pm['loc_conv'].reshape(C, Kf)
    hl = torch.as_tensor(hlens).long()
    frames = torch.arange(T).unsqueeze(0)
    w = ((frames < hl.unsqueeze(1)).to(hmask.dtype) / hl.unsqueeze(1).to(hmask.dtype))
    z = hmask.new_zeros(B, D)
    c = hmask.new_zeros(B, D)
    bias = Pm['b_ih'] + Pm['b_hh']
    zs, ws = [], []
    for i in range(L1):
        windows = F.pad(w, (Fh, Fh)).unfold(1, Kf, 1)                              # (B,T,Kf): windows[b,t,k] = w[b, t + k - Fh]
        conv = windows @ taps.t()                                                  # (B,T,C)
        inner = conv @ Pm['mlp_att'].t() + pre + (z @ Pm['mlp_dec'].t()).unsqueeze(1)
        e = (torch.tanh(inner) * Pm['gvec_w'].reshape(1, 1, -1)).sum(2) + Pm['gvec_b']
        w = torch.softmax(2.0 * e, dim=1)
        ctx = (w.unsqueeze(2) * hmask).sum(1)
        x = torch.cat([Pm['embed'][ids[i].long()], ctx], 1)
        gi, gf, gg, go = (x @ Pm['w_ih'].t() + z @ Pm['w_hh'].t() + bias).chunk(4, 1)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        z = torch.sigmoid(go) * torch.tanh(c)
        zs.append(z)
        ws.append(w)
    return torch.stack(zs, 0), torch.stack(ws, 0)


# (B, T, L1, E, A, D, C, Fh), what the persistent form (csrc/decloop.hip) takes of it, why the shape is here
DEC_SHAPES = [
    ((2, 33, 3, 68, 65, 20, 5, 8), 'none', 'two frame chunks with a one-frame tail, A one past a slice, E one float4 past a context block, D with a '
                                           '16-unroll trip plus remainder per quarter, Kf = 17, one full channel group (A % 4: stepwise only)'),
    ((3, 300, 4, 132, 68, 36, 12, 7), 'fwd', 'two chunks, E and A in different slice counts (E % 16: the persistent backward declines)'),
    ((2, 40, 3, 64, 64, 16, 12, 100), 'both', 'more taps than frames, CMAX channels, three channel groups'),
    ((1, 5, 1, 16, 4, 4, 1, 0), 'both', 'one of everything, one tap'),
    ((3, 70, 5, 512, 320, 300, 10, 100), 'both', 'production widths on three chunks'),
    ((5, 37, 6, 32, 24, 12, 3, 4), 'both', 'ragged, C = 3 (cpad), hlens down to T/2'),
]
DEC_KEYS = ('embed', 'w_ih', 'w_hh', 'b_ih', 'b_hh', 'mlp_dec', 'mlp_att', 'loc_conv', 'gvec_w', 'gvec_b')


def decoder_case(shape):
    """Inputs at the weight scales of test_decoder_loop_persistent_vs_stepwise; upstream gradients ``gz`` on the states and ``gw`` on the
    attention weights."""
    B, T, L1, E, A, D, C, Fh = shape
    g = torch.Generator().manual_seed(B * 1000 + T + 7)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    hl = torch.randint(max(1, T // 2), T + 1, (B,), generator=g)
    hl[0] = T
    if B > 1:
        hl[B - 1] = max(1, T // 2)
    hmask = r(B, T, E)
    for b in range(B):
        hmask[b, int(hl[b]):] = 0
    pre = r(B, T, A)
    Pm = dict(embed=r(50, D, scale=0.5), w_ih=r(4 * D, D + E, scale=0.08), w_hh=r(4 * D, D, scale=0.08), b_ih=r(4 * D, scale=0.1), b_hh=r(4 * D, scale=0.1),
              mlp_dec=r(A, D, scale=0.1), mlp_att=r(A, C, scale=0.5), loc_conv=r(C, 1, 1, 2 * Fh + 1, scale=0.3), gvec_w=r(1, A, scale=0.3), gvec_b=r(1, scale=0.1))
    ids = torch.randint(0, 50, (L1, B), generator=g).to(torch.int32)
    return dict(hmask=hmask, pre=pre, Pm=Pm, ids=ids, hlens=[int(v) for v in hl], gz=r(L1, B, D), gw=r(L1, B, T), L1=L1)


DEC_UPSTREAM = ('zs', 'zs+w')      # upstream gradient on the states alone (all the model uses) / on the states and on the attention weights


def decoder_ref_run(case, dtype=torch.float64, upstream='zs'):
    """decoder_loop_ref and its gradients under the case's upstream gradient(s) -> dict of detached tensors (zs, w, d_enc, d_pre, every Pm key)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)       # (a copy: the case's own tensors stay as they are)
    hm, pr = leaf(case['hmask']), leaf(case['pre'])
    Pm = {k: leaf(v) for k, v in case['Pm'].items()}
    zs, w = decoder_loop_ref(hm, pr, case['ids'], case['hlens'], case['L1'], Pm)
    assert upstream in DEC_UPSTREAM
    up = (zs * case['gz'].to(dtype)).sum()
    if upstream == 'zs+w':
        up = up + (w * case['gw'].to(dtype)).sum()
    up.backward()
    out = dict(zs=zs.detach(), w=w.detach(), d_enc=hm.grad, d_pre=pr.grad)
    out.update({k: v.grad for k, v in Pm.items()})
    return out
