#!/usr/bin/env python3
"""Training the RNNLM: milliseconds per truncated-BPTT window and words per second, with the recurrence on the fused step kernels of
csrc/lmseq.hip and on the composed sequence (model/lm.py COMPOSED_PATH: re2e_gemm + re2e_lstm_cell_fwd / _bwd per step -- kernels the
library had before lmseq.hip).

The recipe's shape: T = 35, input = hidden = 650 units, V = 4233, at B = 256 and B = 2048, dropout 0.2.  One iteration = what
model/lm.py train() does per window: forward_seq, zero_grad, backward, detach, clip at 5, SGD step.  Before any timing the two arms run
the same window from the same parameters and their losses and gradients are compared (kernel bars: 1e-4 / 2e-4 of the max).  Then the arms
alternate ``--rounds`` times in one process after ``--warmup`` iterations each; an iteration is timed with device events.

    python tools/bench_lm_train.py                               # the table, then the kernel trace of one fused run (rocprofv3, a child process)
    python tools/bench_lm_train.py --no-trace                    # the table only
    python tools/bench_lm_train.py --arm fused --batch 256       # a few iterations of one arm (what the trace runs)
    python tools/bench_lm_train.py --kernel-stats DIR            # share of the step kernels and their achieved FLOP/s from a trace directory"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, I, H, V = 35, 650, 650, 4233
PEAK_F32_MFMA = 157.3e12          # FLOP/s, MI355X fp32-input MFMA (= the fp32 vector peak)
TRACE_ITERS = 4                   # iterations of an --arm run (the first is the warm-up)


def step_flops(B):
    """FLOPs of the step kernels per window, from the shapes: per layer T forward products of (B,H) x (H,4H) and T - 1 backward products of
    (B,4H) x (4H,H) (the state carried in is detached: no dh0 product)."""
    return 2 * (T * 2.0 * B * 4 * H * H + (T - 1) * 2.0 * B * 4 * H * H)


def kernel_stats(path, B):
    files = glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True) if os.path.isdir(path) else [path]
    assert files, 'no *kernel_stats.csv under %s' % path
    rows = list(csv.DictReader(open(files[0])))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    iters = TRACE_ITERS
    for name in ('lmseq_fwd_step', 'lmseq_bwd_step'):
        sel = [r for r in rows if name in r['Name']]
        ns, calls = sum(float(r['TotalDurationNs']) for r in sel), sum(int(r['Calls']) for r in sel)
        steps = 2 * iters * (T if 'fwd' in name else T - 1)
        flops = steps * 2.0 * B * 4 * H * H
        # (the backward's launch at t = T - 1 has no product: it is in the calls and the time, not in the FLOPs)
        print('%-16s calls %5d  average %8.2f us  %5.1f %% of kernel time  %6.2f TFLOP/s = %4.1f %% of the fp32 MFMA peak'
              % (name, calls, ns / max(calls, 1) / 1e3, 100 * ns / total, flops / ns / 1e3, 100 * flops / (ns * 1e-9) / PEAK_F32_MFMA))
    print('ten largest kernels of the trace:')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:10]:
        print('  %5.1f %%  calls %5d  average %9.2f us  %s' % (100 * float(r['TotalDurationNs']) / total, int(r['Calls']), float(r['AverageNs']) / 1e3, r['Name'][:90]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 2048])
    ap.add_argument('--batch', type=int, default=256, help='with --arm / --kernel-stats: the batch size')
    ap.add_argument('--rounds', type=int, default=9, help='alternations of the two arms')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--arm', choices=('fused', 'composed'), default=None, help='run only this arm, %d iterations (for a kernel trace)' % TRACE_ITERS)
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-dir', default=None, help='where rocprofv3 writes its trace (default: a fresh temporary directory)')
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.batch)

    import numpy as np
    import torch
    from robust_e2e_gan_amd import lib, ops
    from robust_e2e_gan_amd.model import lm as lm_mod
    from robust_e2e_gan_amd.optim import FlatOptimizer
    assert torch.cuda.is_available() and lib.query('re2e_device_ok') == 1, 'needs an MI355X: there is nothing to measure on a CPU'
    dev = 'cuda:0'

    def make(seed=3):
        torch.manual_seed(seed)
        m = lm_mod.ClassifierWithState(lm_mod.RNNLM(V, I, H, dropout_rate=0.2))
        m.compute_accuracy = False
        return m.to(dev).train()

    def window(B, seed):
        rng = np.random.RandomState(seed)
        return rng.randint(0, V, (T, B)).astype(np.int32), rng.randint(0, V, (T, B)).astype(np.int32)

    class Arm(object):
        def __init__(self, composed, B):
            self.composed, self.B = composed, B
            self.model = make()
            self.opt = FlatOptimizer(self.model.parameters(), kind='sgd', lr=1.0)
            self.state = None
            self.n = 0

        def iteration(self, timed=True):
            xs, ts = window(self.B, 100 + self.n)
            self.n += 1
            lm_mod.COMPOSED_PATH = self.composed
            try:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                self.state, loss = self.model.forward_seq(self.state, xs, ts)
                self.opt.zero_grad()
                loss.backward()
                self.state = {k: v.detach() for k, v in self.state.items()}
                self.opt.clip_grad_norm(5.0)
                self.opt.step()
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1), float(loss.detach())
            finally:
                lm_mod.COMPOSED_PATH = False

    if a.arm:
        arm = Arm(a.arm == 'composed', a.batch)
        for _ in range(TRACE_ITERS):
            arm.iteration()
        return

    def rel(x, y):
        return float((x.double() - y.double()).abs().max() / y.double().abs().max())

    print('RNNLM training window: T = %d, input = %d, hidden = %d, V = %d, dropout 0.2; %s' % (T, I, H, V, torch.cuda.get_device_name(0)))
    for B in a.batches:
        for backward in (False, True):
            print('plan B=%d %s: %s' % (B, 'bwd' if backward else 'fwd', ' '.join('%s=%s' % kv for kv in lib.lmseq_plan(T, B, H, backward=backward).items())))
        # the arms against each other on one window, same parameters, same dropout masks, non-zero carried state
        got = []
        for composed in (False, True):
            m = make()
            ops.dropout_seed(5, 0)
            lm_mod.COMPOSED_PATH = composed
            xs, ts = window(B, 7)
            state, l0 = m.forward_seq(None, xs, ts)
            state, l1 = m.forward_seq({k: v.detach() for k, v in state.items()}, *window(B, 8))
            m.zero_grad()
            l1.backward()
            lm_mod.COMPOSED_PATH = False
            got.append((l1.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
        worst = max(rel(got[0][1][k], got[1][1][k]) for k in got[0][1])
        print('B=%d fused vs composed: loss %.2e, worst gradient %.2e of the max' % (B, rel(got[0][0], got[1][0]), worst))
        assert rel(got[0][0], got[1][0]) <= 1e-4 and worst <= 2e-4, 'the arms disagree: nothing to time'
        del got, m, state
        arms = {'fused': Arm(False, B), 'composed': Arm(True, B)}
        for name, arm in arms.items():
            for _ in range(max(1, a.warmup)):
                arm.iteration()
        ms = {name: [] for name in arms}
        for _ in range(max(5, a.rounds)):
            for name, arm in arms.items():
                ms[name].append(arm.iteration()[0])
        print('B=%d, %d alternations after %d warm-up iterations each' % (B, max(5, a.rounds), max(1, a.warmup)))
        print('  %-10s %14s %9s %9s %13s %14s' % ('arm', 'median ms/win', 'min', 'max', 'quartiles', 'words/s'))
        med, iqr = {}, {}
        for name, v in ms.items():
            q = statistics.quantiles(v, n=4)
            med[name], iqr[name] = statistics.median(v), q[2] - q[0]
            print('  %-10s %14.2f %9.2f %9.2f %6.2f-%-6.2f %14.0f' % (name, med[name], min(v), max(v), q[0], q[2], T * B / (med[name] * 1e-3)))
        d, spread = med['composed'] - med['fused'], max(iqr.values())
        print('  fused is %.2f ms per window %s than composed (%.2fx) against a spread of %.2f ms (widest interquartile range) -> %s'
              % (abs(d), 'faster' if d > 0 else 'slower', med['composed'] / med['fused'], spread, 'separated' if abs(d) > spread else 'NOT separated from the spread'))
        del arms
        torch.cuda.empty_cache()
    if not a.no_trace:
        # the kernel trace: a run of its own in a fresh process, no counters
        B = a.batches[0]
        trace_dir = a.trace_dir or tempfile.mkdtemp(prefix='lm_train_trace_')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', trace_dir, '--', sys.executable, os.path.abspath(__file__),
               '--arm', 'fused', '--batch', str(B)]
        print('kernel trace (B=%d, %d iterations of the fused arm): %s' % (B, TRACE_ITERS, ' '.join(cmd[:8])))
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        kernel_stats(trace_dir, B)


if __name__ == '__main__':
    main()
