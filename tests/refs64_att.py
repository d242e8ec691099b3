"""Float64 references of the decoder loop for the attention types dot, add, coverage and coverage_location (csrc/attstep.hip; the
coverage_location step is csrc/attloc.hip reading cov), and the inputs of tests/test_attstep_kernels_gpu.py.

Plain torch on the CPU, autograd for every gradient, nothing imported from the product or from ``oracle``; helpers and the input
generator come from refs64.py.  ``att_loop_ref`` is written out from the formulas; ``att_loop_modules`` is a second derivation through
``torch.nn`` modules with the attention state kept as the LIST of weight rows the reference keeps; tests/test_refs64_att_cpu.py pins
both to each other and to the golden vectors of tests/golden/att_types_tiny.npz."""
import torch
import torch.nn.functional as F

import refs64 as R

KINDS = ('dot', 'add', 'coverage', 'coverage_location')
# the parameters of Pm a kind has beside the decoder's (embed, w_ih, w_hh, b_ih, b_hh)
ATT_KEYS = {
    'dot': ('mlp_dec', 'mlp_dec_b'),
    'add': ('mlp_dec', 'gvec_w', 'gvec_b'),
    'coverage': ('mlp_dec', 'wvec_w', 'wvec_b', 'gvec_w', 'gvec_b'),
    'coverage_location': ('mlp_dec', 'mlp_att', 'loc_conv', 'gvec_w', 'gvec_b'),
}
DEC_KEYS = ('embed', 'w_ih', 'w_hh', 'b_ih', 'b_hh')


def cov0(hlens, T, dtype):
    hl = torch.as_tensor(hlens).long()
    return (torch.arange(T).unsqueeze(0) < hl.unsqueeze(1)).to(dtype) / hl.unsqueeze(1).to(dtype)


def _cell(Pm, ids_i, ctx, z, c):
    x = torch.cat([Pm['embed'][ids_i.long()], ctx], 1)
    gi, gf, gg, go = (x @ Pm['w_ih'].t() + z @ Pm['w_hh'].t() + Pm['b_ih'] + Pm['b_hh']).chunk(4, 1)
    c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
    return torch.sigmoid(go) * torch.tanh(c), c


def att_loop_ref(kind, hmask, pre, ids, hlens, L1, Pm, out_w=None, out_b=None, sample_steps=None):
    """hmask (B,T,E) masked encoder states, pre (B,T,A) = mlp_enc(hmask) -- for ``dot`` tanh(mlp_enc(hmask)) --, ids (L1,B) tokens fed
    -> (zs (L1,B,D), w (L1,B,T), ids actually fed).  Step i with z_0 = c_0 = 0, cov_0 = 1/hlen over the valid frames, cov_{i+1} = cov_i + w_i:
        add               e = gvec . tanh(pre + mlp_dec z_i) + gvec_b
        dot               e = sum_a pre[.,.,a] tanh(mlp_dec z_i + mlp_dec_b)[a]
        coverage          e = gvec . tanh(wvec_w cov_i[b,t] + wvec_b + pre + mlp_dec z_i) + gvec_b
        coverage_location e = gvec . tanh(mlp_att conv(cov_i) + pre + mlp_dec z_i) + gvec_b      (AttLoc's energy on cov_i)
        w_i = softmax over ALL T frames of 2 e,  ctx = sum_t w_i[b,t] hmask[b,t],  then the LSTMCell of refs64.decoder_loop_ref.
    ``sample_steps`` (with out_w / out_b): step i > 0 with sample_steps[i] feeds the arg-max (lowest index) of output(z_i)."""
    assert kind in KINDS
    B, T, E = hmask.shape
    D = Pm['w_hh'].shape[1]
    cov = cov0(hlens, T, hmask.dtype)
    z, c = hmask.new_zeros(B, D), hmask.new_zeros(B, D)
    ids = ids.clone()
    zs, ws = [], []
    for i in range(L1):
        if sample_steps is not None and i > 0 and sample_steps[i]:
            ids[i] = R.argmax_first((z @ out_w.t() + out_b).detach()).to(ids.dtype)
        dp = (z @ Pm['mlp_dec'].t()).unsqueeze(1)
        if kind == 'dot':
            e = (pre * torch.tanh(dp + Pm['mlp_dec_b'])).sum(2)
        else:
            if kind == 'add':
                inner = pre + dp
            elif kind == 'coverage':
                inner = cov.unsqueeze(2) * Pm['wvec_w'].reshape(1, 1, -1) + Pm['wvec_b'] + pre + dp
            else:
                C, Kf = Pm['loc_conv'].shape[0], Pm['loc_conv'].shape[3]
                Fh = (Kf - 1) // 2
                windows = F.pad(cov, (Fh, Fh)).unfold(1, Kf, 1)                      # (B,T,Kf): cov[b, t + k - Fh]
                inner = (windows @ Pm['loc_conv'].reshape(C, Kf).t()) @ Pm['mlp_att'].t() + pre + dp
            e = (torch.tanh(inner) * Pm['gvec_w'].reshape(1, 1, -1)).sum(2) + Pm['gvec_b']
        w = torch.softmax(2.0 * e, dim=1)
        cov = cov + w
        ctx = (w.unsqueeze(2) * hmask).sum(1)
        z, c = _cell(Pm, ids[i], ctx, z, c)
        zs.append(z)
        ws.append(w)
    return torch.stack(zs, 0), torch.stack(ws, 0), ids


def att_loop_modules(kind, hmask, pre, ids, hlens, L1, Pm):
    """The same loop through torch.nn modules (Linear, Conv2d, LSTMCell, Embedding) holding Pm's tensors, with the coverage state as the
    list of weight rows that is summed at every step -> (zs, w, dict of the modules' parameters by Pm key)."""
    B, T, E = hmask.shape
    dt = hmask.dtype
    D, Dd, A = Pm['w_hh'].shape[1], Pm['embed'].shape[1], Pm['mlp_dec'].shape[0]

    def lin(w, b=None):
        m = torch.nn.Linear(w.shape[1], w.shape[0], bias=b is not None).to(dt)
        m.weight.data.copy_(w)
        if b is not None:
            m.bias.data.copy_(b)
        return m

    embed = torch.nn.Embedding(*Pm['embed'].shape).to(dt)
    embed.weight.data.copy_(Pm['embed'])
    cell = torch.nn.LSTMCell(Dd + E, D).to(dt)
    for n, k in (('weight_ih', 'w_ih'), ('weight_hh', 'w_hh'), ('bias_ih', 'b_ih'), ('bias_hh', 'b_hh')):
        getattr(cell, n).data.copy_(Pm[k])
    params = dict(embed=embed.weight, w_ih=cell.weight_ih, w_hh=cell.weight_hh, b_ih=cell.bias_ih, b_hh=cell.bias_hh)
    mlp_dec = lin(Pm['mlp_dec'], Pm.get('mlp_dec_b'))
    params['mlp_dec'] = mlp_dec.weight
    if kind == 'dot':
        params['mlp_dec_b'] = mlp_dec.bias
    else:
        gvec = lin(Pm['gvec_w'], Pm['gvec_b'])
        params.update(gvec_w=gvec.weight, gvec_b=gvec.bias)
    if kind == 'coverage':
        wvec = lin(Pm['wvec_w'], Pm['wvec_b'])
        params.update(wvec_w=wvec.weight, wvec_b=wvec.bias)
    if kind == 'coverage_location':
        C, Kf = Pm['loc_conv'].shape[0], Pm['loc_conv'].shape[3]
        conv = torch.nn.Conv2d(1, C, (1, Kf), padding=(0, (Kf - 1) // 2), bias=False).to(dt)
        conv.weight.data.copy_(Pm['loc_conv'])
        mlp_att = lin(Pm['mlp_att'])
        params.update(loc_conv=conv.weight, mlp_att=mlp_att.weight)
    prev = [cov0(hlens, T, dt)]
    z, c = hmask.new_zeros(B, D), hmask.new_zeros(B, D)
    zs, ws = [], []
    for i in range(L1):
        dz = mlp_dec(z).view(B, 1, A)
        if kind == 'dot':
            e = torch.sum(pre * torch.tanh(dz), dim=2)
        elif kind == 'add':
            e = gvec(torch.tanh(pre + dz)).squeeze(2)
        elif kind == 'coverage':
            e = gvec(torch.tanh(wvec(sum(prev).unsqueeze(-1)) + pre + dz)).squeeze(2)
        else:
            ac = conv(sum(prev).view(B, 1, 1, T)).squeeze(2).transpose(1, 2)
            e = gvec(torch.tanh(mlp_att(ac) + pre + dz)).squeeze(2)
        w = F.softmax(2.0 * e, dim=1)
        prev.append(w)
        ctx = torch.sum(hmask * w.view(B, T, 1), dim=1)
        z, c = cell(torch.cat((embed(ids[i].long()), ctx), dim=1), (z, c))
        zs.append(z)
        ws.append(w)
    return torch.stack(zs, 0), torch.stack(ws, 0), params


# (B, T, L1, E, A, D, C, Fh) -- C and Fh are read by coverage_location alone -- and why the shape is here.  The kernels' break points:
# frame chunks of 32 (energies, step backward) and of 16 (the after-loop pass), 64-lane slices of A (at most five), 64-column context
# blocks of E read as float4, the softmax pass striding T by 256 threads, four quarters of D in the decoder projection.
ATT_SHAPES = [
    ((1, 5, 1, 16, 4, 4, 1, 0), 'one of everything'),
    ((2, 1, 2, 4, 4, 4, 1, 0), 'one frame: w = 1 at every step, cov = 1 + i'),
    ((2, 33, 3, 68, 65, 20, 5, 8), 'chunk tail of one frame, A one past a slice, E one float4 past a context block'),
    ((5, 37, 6, 32, 24, 12, 3, 4), 'ragged lengths, six steps of coverage carry'),
    ((3, 300, 4, 132, 68, 36, 12, 7), 'E and A in different slice counts, T past one stride of the softmax pass (256 threads)'),
    ((3, 70, 5, 512, 320, 300, 10, 100), 'production widths: all five slices of A full'),
    ((2, 64, 2, 64, 64, 16, 2, 1), 'everything exactly one tile: two full 32-frame chunks, four 16-frame chunks, one slice of A, one context block'),
    ((2, 17, 3, 8, 129, 68, 1, 2), 'A one past two slices, one frame past a 16-frame chunk of the after-loop pass, D with a full 16-unroll trip per quarter'),
]


def att_case(kind, shape):
    """refs64.decoder_case on the shape plus the parameters only this kind has (mlp_dec_b ~ 0.1, wvec_w ~ 0.5, wvec_b ~ 0.1); Pm holds
    exactly the kind's keys."""
    B, T, L1, E, A, D, C, Fh = shape
    c = dict(R.decoder_case(shape))
    g = torch.Generator().manual_seed(B * 1000 + T + 77)
    extra = dict(mlp_dec_b=R.rnd(g, A, scale=0.1), wvec_w=R.rnd(g, A, 1, scale=0.5), wvec_b=R.rnd(g, A, scale=0.1))
    full = dict(c['Pm'], **extra)
    c['Pm'] = {k: full[k] for k in DEC_KEYS + ATT_KEYS[kind]}
    c['kind'] = kind
    if kind == 'dot':
        c['pre'] = torch.tanh(c['pre'])             # what the caller hands the loop: tanh(mlp_enc(h))
    return c


def att_ref_run(case, dtype=torch.float64, upstream='zs', loop=att_loop_ref):
    """The loop and its gradients under the case's upstream gradient(s) -> dict of detached tensors (zs, w, d_enc, d_pre, every Pm key)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    hm, pr = leaf(case['hmask']), leaf(case['pre'])
    Pm = {k: leaf(v) for k, v in case['Pm'].items()}
    out = loop(case['kind'], hm, pr, case['ids'], case['hlens'], case['L1'], Pm)
    zs, w = out[0], out[1]
    grads_of = Pm if loop is att_loop_ref else out[2]
    assert upstream in R.DEC_UPSTREAM
    up = (zs * case['gz'].to(dtype)).sum()
    if upstream == 'zs+w':
        up = up + (w * case['gw'].to(dtype)).sum()
    up.backward()
    res = dict(zs=zs.detach(), w=w.detach(), d_enc=hm.grad, d_pre=pr.grad)
    res.update({k: grads_of[k].grad for k in Pm})
    return res
