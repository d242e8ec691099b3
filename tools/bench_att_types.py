#!/usr/bin/env python3
"""The decoder loop and the beam-search position of the attention types dot, add, coverage and coverage_location, alone on the chip:

  loop      ops.DecoderLoopFn at the flagship decoder shape (B=32, T'=200, E=512, A=320, D=300, L+1=41), forward and forward+backward,
            every new kind against ``location`` on the launch-per-step path (ops.DECODER_PERSIST = False) and on the persistent path, and
            against the same loop composed of torch ops on the GPU (autograd backward)
  recognize Decoder.recognize_beam at beam 12 on one utterance of T' = 200 frames, attention-only, 40 positions: milliseconds per
            position, the HIP step against the same search with the attention step composed of torch ops

All arms run in one process, alternated round by round; the table gives the median over the rounds and their (min .. max) spread.
    python tools/bench_att_types.py [--rounds 7] [--out profiles/att_types.md]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from robust_e2e_gan_amd import ops, lib

DEV = 'cuda:0'
KINDS = ('location', 'dot', 'add', 'coverage', 'coverage_location')
ATT_KEYS = {'location': ('mlp_dec', 'mlp_att', 'loc_conv', 'gvec_w', 'gvec_b'), 'coverage_location': ('mlp_dec', 'mlp_att', 'loc_conv', 'gvec_w', 'gvec_b'),
            'add': ('mlp_dec', 'gvec_w', 'gvec_b'), 'coverage': ('mlp_dec', 'wvec_w', 'wvec_b', 'gvec_w', 'gvec_b'), 'dot': ('mlp_dec', 'mlp_dec_b')}


def torch_step(kind, ap, pre, enc, z, state, hl):
    """One attention step in torch ops -> (context, weights, new state); state: previous weights (location) / cov (coverage types)."""
    T = pre.shape[1]
    if state is None and kind not in ('dot', 'add'):
        state = (torch.arange(T, device=pre.device).unsqueeze(0) < hl.unsqueeze(1)).to(pre.dtype) / hl.unsqueeze(1).to(pre.dtype)
    dp = (z @ ap['mlp_dec'].t()).unsqueeze(1)
    if kind == 'dot':
        e = (pre * torch.tanh(dp + ap['mlp_dec_b'])).sum(2)
    else:
        if kind == 'add':
            inner = pre + dp
        elif kind == 'coverage':
            inner = state.unsqueeze(2) * ap['wvec_w'].reshape(1, 1, -1) + ap['wvec_b'] + pre + dp
        else:
            Fh = (ap['loc_conv'].shape[3] - 1) // 2
            conv = F.conv2d(state.view(-1, 1, 1, T), ap['loc_conv'], padding=(0, Fh)).squeeze(2).transpose(1, 2)
            inner = conv @ ap['mlp_att'].t() + pre + dp
        e = (torch.tanh(inner) * ap['gvec_w'].reshape(1, 1, -1)).sum(2) + ap['gvec_b']
    w = torch.softmax(2.0 * e, dim=1)
    cx = torch.bmm(w.unsqueeze(1), enc).squeeze(1)
    new = None if kind in ('dot', 'add') else (w if kind == 'location' else state + w)
    return cx, w, new


def torch_loop(kind, hmask, pre, ids, hl, L1, Pm):
    B, D = hmask.shape[0], Pm['w_hh'].shape[1]
    z, c, state = hmask.new_zeros(B, D), hmask.new_zeros(B, D), None
    emb = Pm['embed'][ids.long()]
    bias = Pm['b_ih'] + Pm['b_hh']
    zs = []
    for i in range(L1):
        cx, w, state = torch_step(kind, Pm, pre, hmask, z, state, hl)
        gi, gf, gg, go = (torch.cat([emb[i], cx], 1) @ Pm['w_ih'].t() + z @ Pm['w_hh'].t() + bias).chunk(4, 1)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        z = torch.sigmoid(go) * torch.tanh(c)
        zs.append(z)
    return torch.stack(zs, 0)


def loop_case(kind, B=32, T=200, L1=41, E=512, A=320, D=300, C=10, Fh=100):
    g = torch.Generator().manual_seed(1)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    hmask, pre = r(B, T, E).requires_grad_(True), r(B, T, A).requires_grad_(True)
    full = dict(embed=r(50, D, scale=0.5), w_ih=r(4 * D, D + E, scale=0.08), w_hh=r(4 * D, D, scale=0.08), b_ih=r(4 * D, scale=0.1), b_hh=r(4 * D, scale=0.1),
                mlp_dec=r(A, D, scale=0.1), mlp_att=r(A, C, scale=0.5), loc_conv=r(C, 1, 1, 2 * Fh + 1, scale=0.3), gvec_w=r(1, A, scale=0.3),
                gvec_b=r(1, scale=0.1), mlp_dec_b=r(A, scale=0.1), wvec_w=r(A, 1, scale=0.5), wvec_b=r(A, scale=0.1))
    Pm = {k: torch.nn.Parameter(full[k]) for k in ('embed', 'w_ih', 'w_hh', 'b_ih', 'b_hh') + ATT_KEYS[kind]}
    ids = torch.randint(0, 50, (L1, B), generator=g).to(torch.int32).to(DEV)
    hlens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    return hmask, pre, ids, hlens, L1, Pm


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def bench_loop(rounds, reps):
    arms = {}
    for kind in KINDS:
        hmask, pre, ids, hlens, L1, Pm = loop_case(kind)

        def hip(bwd, persist, kind=kind, a=(hmask, pre, ids, hlens, L1, Pm)):
            ops.DECODER_PERSIST = persist
            if bwd:
                z, _ = ops.DecoderLoopFn.apply(*a, None, False, kind)
                z.sum().backward()
            else:
                with torch.no_grad():
                    ops.DecoderLoopFn.apply(*a, None, False, kind)

        def tor(bwd, kind=kind, a=(hmask, pre, ids, hlens, L1, Pm)):
            if bwd:
                torch_loop(kind, *a).sum().backward()
            else:
                with torch.no_grad():
                    torch_loop(kind, *a)

        for bwd in (False, True):
            d = 'fwd+bwd' if bwd else 'fwd'
            arms[(kind, 'hip launch-per-step', d)] = lambda bwd=bwd, hip=hip: hip(bwd, False)
            if kind == 'location':
                arms[(kind, 'hip persistent', d)] = lambda bwd=bwd, hip=hip: hip(bwd, True)
            arms[(kind, 'torch ops', d)] = lambda bwd=bwd, tor=tor: tor(bwd)
    was = ops.DECODER_PERSIST
    res = {k: [] for k in arms}
    try:
        for fn in arms.values():
            fn()                                    # warm every arm's shapes
        for _ in range(rounds):
            for k, fn in arms.items():
                res[k].append(timed(fn, reps))
    finally:
        ops.DECODER_PERSIST = was
    return res


def bench_recognize(rounds, positions=40, beam=12, T=200):
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model import beam_search
    from robust_e2e_gan_amd.model.e2e_model import E2E
    res = {}
    models = {}
    for kind in KINDS:
        opt = config4_opt(odim=52, char_list=[str(i) for i in range(52)])
        opt.atype = kind
        torch.manual_seed(3)
        models[kind] = E2E(opt).to(DEV).eval()
    h = torch.randn(T, models['location'].opt.eprojs, generator=torch.Generator().manual_seed(5)).to(DEV)
    args = argparse.Namespace(beam_size=beam, penalty=0.0, ctc_weight=0.0, maxlenratio=positions / T, minlenratio=0.0, nbest=1, lm_weight=0.0)
    hip_step = beam_search._att_step
    count = [0]

    def counted(*a, **kw):
        count[0] += 1
        return hip_step(*a, **kw)

    def composed(kind, ap, pre, enc, z, state, hl, w_decT, nh, T_, E, D, A, utt=None, U=0):
        count[0] += 1
        cx, _, new = torch_step(kind, ap, pre[:nh], enc[:nh], z, state, hl[:nh])
        return cx.contiguous(), (new.contiguous() if new is not None else None)

    def run(kind, step):
        beam_search._att_step = step
        count[0] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        models[kind].dec.recognize_beam(h, None, args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / max(count[0], 1), count[0]

    try:
        for kind in KINDS:
            for name, step in (('hip', counted), ('torch ops step', composed)):
                run(kind, step)
        for _ in range(rounds):
            for kind in KINDS:
                for name, step in (('hip', counted), ('torch ops step', composed)):
                    ms, n = run(kind, step)
                    res.setdefault((kind, name), []).append(ms)
                    res.setdefault((kind, name, 'positions'), []).append(n)
    finally:
        beam_search._att_step = hip_step
    return res


def fmt(v):
    return '%.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'att_types.md'))
    a = ap.parse_args()
    assert torch.cuda.is_available() and lib.query('re2e_device_ok') == 1, 'needs a gfx950 device: nothing is measured without one'
    loop = bench_loop(a.rounds, a.reps)
    rec = bench_recognize(a.rounds)
    out = ['## Measured (tools/bench_att_types.py, %d alternated rounds; median (min .. max), milliseconds)' % a.rounds, '',
           '### Decoder loop alone, B=32, T\'=200, E=512, A=320, D=300, L+1=41 (%d loops per timing)' % a.reps, '',
           '| atype | arm | forward | forward+backward |', '|---|---|---|---|']
    for kind in KINDS:
        for arm in ('hip launch-per-step', 'hip persistent', 'torch ops'):
            if (kind, arm, 'fwd') in loop:
                out.append('| %s | %s | %s | %s |' % (kind, arm, fmt(loop[(kind, arm, 'fwd')]), fmt(loop[(kind, arm, 'fwd+bwd')])))
    out += ['', '### recognize, beam 12, T\'=200, attention only: milliseconds per output position', '',
            '| atype | positions | HIP step | attention step in torch ops |', '|---|---|---|---|']
    for kind in KINDS:
        out.append('| %s | %d | %s | %s |' % (kind, rec[(kind, 'hip', 'positions')][0], fmt(rec[(kind, 'hip')]), fmt(rec[(kind, 'torch ops step')])))
    text = '\n'.join(out) + '\n'
    print(text)
    # the tables replace what stands between the two markers of the file (its commentary stays); a new file is the markers and the tables
    begin, end = '<!-- measured: begin -->\n', '<!-- measured: end -->\n'
    old = open(a.out).read() if os.path.exists(a.out) else '# Attention types dot, add, coverage, coverage_location: measurements\n\n' + begin + end
    assert begin in old and end in old, '%s has lost its markers' % a.out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(old[:old.index(begin) + len(begin)] + text + old[old.index(end):])


if __name__ == '__main__':
    main()
