#!/usr/bin/env python3
"""The multi-layer attention decoder (dlayers 1, 2, 3, ``location``), alone on the chip:

  loop      the decoder loop at the flagship decoder shape (B=32, T'=200, E=512, A=320, D=300, L+1=41), forward and forward+backward:
            (a) ``hip``       ops.DecoderLoopFn (layer 0, persistent) + ops.DecoderUpperFn (csrc/decstack.hip)
            (b) ``composed``  the same layer 0, the upper layers over the entry points that existed before csrc/decstack.hip: forward
                              re2e_dec_gates_cell_fwd per token with z_below in the context slot (gates pre-filled with the biases), backward
                              re2e_lstm_cell_bwd + re2e_gemm_skinny2 per token (d z_below and the carried d z from one launch), the same
                              whole-sequence weight-gradient products behind it
            (c) ``torch ops`` the whole stacked loop composed of torch ops on the GPU (autograd backward)
            dlayers = 1 has no upper layers: (a) and (b) are the same call there and one row is printed.
  recognize Decoder.recognize_beam at beam 12 on one utterance of T' = 200 frames, attention-only, 40 positions: milliseconds per position

All arms run in one process, alternated round by round; the table gives the median over the rounds and their (min .. max) spread.
    python tools/bench_dlayers.py [--rounds 7] [--out profiles/dlayers.md]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from robust_e2e_gan_amd import ops, lib
from robust_e2e_gan_amd.lib import call
from bench_att_types import loop_case, timed, torch_loop

DEV = 'cuda:0'
DLAYERS = (1, 2, 3)


class ComposedUpperFn(torch.autograd.Function):
    """ops.DecoderUpperFn over the entry points of the parent commit (arm (b)); B <= 32 (re2e_gemm_skinny2)."""

    @staticmethod
    def forward(ctx, z0, lays):
        L1, B, D = z0.shape
        bufs, below = [], z0
        for lay in lays:
            gates = (lay['b_ih'].detach() + lay['b_hh'].detach()).expand(L1, B, 4 * D).contiguous()
            z, c = ops.zeros((L1 + 1, B, D), z0), ops.zeros((L1 + 1, B, D), z0)
            for i in range(L1):
                call('re2e_dec_gates_cell_fwd', below[i].data_ptr(), z[i].data_ptr(), lay['w_ih'].data_ptr(), D, lay['w_hh'].data_ptr(), gates[i].data_ptr(),
                     c[i].data_ptr(), c[i + 1].data_ptr(), z[i + 1].data_ptr(), B, D, D)
            bufs.append((gates, z, c))
            below = z[1:]
        ctx.lays, ctx.dims = lays, (L1, B, D)
        ctx.save_for_backward(z0, *[t for b in bufs for t in b])
        return bufs[-1][1][1:]

    @staticmethod
    def backward(ctx, dZ):
        saved = ctx.saved_tensors
        z0, flat = saved[0], saved[1:]
        L1, B, D = ctx.dims
        M = L1 * B
        dZ = dZ.contiguous()
        for l in range(len(ctx.lays) - 1, -1, -1):
            lay = ctx.lays[l]
            gates, z, c = flat[3 * l:3 * l + 3]
            below = flat[3 * (l - 1) + 1][1:] if l > 0 else z0
            d_below = ops.empty((L1, B, D), dZ)
            dz_carry = ops.zeros((B, D), dZ)
            dc_a, dc_b = ops.zeros((B, D), dZ), ops.empty((B, D), dZ)
            for i in range(L1 - 1, -1, -1):
                call('re2e_lstm_cell_bwd', gates[i].data_ptr(), c[i].data_ptr(), c[i + 1].data_ptr(), dz_carry.data_ptr(), dZ[i].data_ptr(), dc_a.data_ptr(),
                     dc_b.data_ptr(), B, D)
                dc_a, dc_b = dc_b, dc_a
                call('re2e_gemm_skinny2', B, 4 * D, gates[i].data_ptr(), 4 * D, lay['w_ih'].data_ptr(), D, D, d_below[i].data_ptr(), D,
                     lay['w_hh'].data_ptr(), D, D, dz_carry.data_ptr(), D)
            G2 = gates.view(M, 4 * D)
            with ops.param_grads(gates, below, z):
                with ops.accumulate(lay['w_ih']) as (gw, beta):
                    ops.gemm(G2, below, gw, 4 * D, D, M, transa=True, beta=beta)
                with ops.accumulate(lay['w_hh']) as (gw, beta):
                    ops.gemm(G2, z, gw, 4 * D, D, M, transa=True, beta=beta)
                for k in ('b_ih', 'b_hh'):
                    with ops.accumulate(lay[k]) as (gb, beta):
                        ops.colsum_into(G2, M, 4 * D, gb, beta)
            dZ = d_below
        return dZ, None


def torch_upper(z0, lays):
    L1, B, D = z0.shape
    below = z0
    for lay in lays:
        z, c = z0.new_zeros(B, D), z0.new_zeros(B, D)
        bias = lay['b_ih'] + lay['b_hh']
        zs = []
        for i in range(L1):
            gi, gf, gg, go = (below[i] @ lay['w_ih'].t() + z @ lay['w_hh'].t() + bias).chunk(4, 1)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            z = torch.sigmoid(go) * torch.tanh(c)
            zs.append(z)
        below = torch.stack(zs, 0)
    return below


def upper_params(n, D):
    g = torch.Generator().manual_seed(2)
    r = lambda *s, scale=1.0: torch.nn.Parameter((torch.randn(*s, generator=g) * scale).to(DEV))
    return [dict(w_ih=r(4 * D, D, scale=0.08), w_hh=r(4 * D, D, scale=0.08), b_ih=r(4 * D, scale=0.1), b_hh=r(4 * D, scale=0.1)) for _ in range(n)]


def bench_loop(rounds, reps):
    arms = {}
    for nl in DLAYERS:
        a = loop_case('location')
        lays = upper_params(nl - 1, a[5]['w_hh'].shape[1])

        def hip(bwd, upper_fn, a=a, lays=lays):
            with torch.set_grad_enabled(bwd):
                z, _ = ops.DecoderLoopFn.apply(*a)
                if lays:
                    z = upper_fn(z, lays)
                if bwd:
                    z.sum().backward()

        def tor(bwd, a=a, lays=lays):
            with torch.set_grad_enabled(bwd):
                z = torch_upper(torch_loop('location', *a), lays)
                if bwd:
                    z.sum().backward()

        for bwd in (False, True):
            d = 'fwd+bwd' if bwd else 'fwd'
            arms[(nl, 'hip', d)] = lambda bwd=bwd, hip=hip: hip(bwd, ops.DecoderUpperFn.apply)
            if nl > 1:
                arms[(nl, 'composed', d)] = lambda bwd=bwd, hip=hip: hip(bwd, ComposedUpperFn.apply)
            arms[(nl, 'torch ops', d)] = lambda bwd=bwd, tor=tor: tor(bwd)
    res = {k: [] for k in arms}
    for fn in arms.values():
        fn()                                    # warm every arm's shapes
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, reps))
    return res


def bench_recognize(rounds, positions=40, beam=12, T=200):
    from robust_e2e_gan_amd.joint_train import config4_opt
    from robust_e2e_gan_amd.model import beam_search
    from robust_e2e_gan_amd.model.e2e_model import E2E
    res, models = {}, {}
    for nl in DLAYERS:
        opt = config4_opt(odim=52, char_list=[str(i) for i in range(52)])
        opt.dlayers = nl
        torch.manual_seed(3)
        models[nl] = E2E(opt).to(DEV).eval()
    h = torch.randn(T, models[1].opt.eprojs, generator=torch.Generator().manual_seed(5)).to(DEV)
    args = argparse.Namespace(beam_size=beam, penalty=0.0, ctc_weight=0.0, maxlenratio=positions / T, minlenratio=0.0, nbest=1, lm_weight=0.0)
    hip_step = beam_search._att_step
    count = [0]

    def counted(*a, **kw):
        count[0] += 1
        return hip_step(*a, **kw)

    def run(nl):
        count[0] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        models[nl].dec.recognize_beam(h, None, args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / max(count[0], 1), count[0]

    beam_search._att_step = counted
    try:
        for nl in DLAYERS:
            run(nl)
        for _ in range(rounds):
            for nl in DLAYERS:
                ms, n = run(nl)
                res.setdefault(nl, []).append(ms)
                res.setdefault((nl, 'positions'), []).append(n)
    finally:
        beam_search._att_step = hip_step
    return res


def fmt(v):
    return '%.3f (%.3f .. %.3f)' % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'dlayers.md'))
    a = ap.parse_args()
    assert torch.cuda.is_available() and lib.query('re2e_device_ok') == 1, 'needs a gfx950 device: nothing is measured without one'
    loop = bench_loop(a.rounds, a.reps)
    rec = bench_recognize(a.rounds)
    out = ['## Measured (tools/bench_dlayers.py, %d alternated rounds; median (min .. max), milliseconds)' % a.rounds, '',
           '### Decoder loop alone, location, B=32, T\'=200, E=512, A=320, D=300, L+1=41 (%d loops per timing)' % a.reps, '',
           '| dlayers | arm | forward | forward+backward |', '|---|---|---|---|']
    for nl in DLAYERS:
        for arm in ('hip', 'composed', 'torch ops'):
            if (nl, arm, 'fwd') in loop:
                out.append('| %d | %s | %s | %s |' % (nl, arm, fmt(loop[(nl, arm, 'fwd')]), fmt(loop[(nl, arm, 'fwd+bwd')])))
    out += ['', '### recognize, beam 12, T\'=200, attention only: milliseconds per output position', '',
            '| dlayers | positions | HIP |', '|---|---|---|']
    for nl in DLAYERS:
        out.append('| %d | %d | %s |' % (nl, rec[(nl, 'positions')][0], fmt(rec[nl])))
    text = '\n'.join(out) + '\n'
    print(text)
    # the tables replace what stands between the two markers of the file (its commentary stays); a new file is the markers and the tables
    begin, end = '<!-- measured: begin -->\n', '<!-- measured: end -->\n'
    old = open(a.out).read() if os.path.exists(a.out) else '# Multi-layer attention decoder (dlayers > 1): measurements\n\n' + begin + end
    assert begin in old and end in old, '%s has lost its markers' % a.out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(old[:old.index(begin) + len(begin)] + text + old[old.index(end):])


if __name__ == '__main__':
    main()
